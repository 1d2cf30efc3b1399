"""Camera helpers with the call surface of the reference's utils/cam_utils.py that a training step needs.  Plain tensor operations on
the device (glue between the SMPL joints and the 2D-joint loss, a few thousand numbers; autograd differentiates them as they are)."""
import torch


def orthographic_project_torch(points3D, cam_params):
    """utils/cam_utils.py:9-16: scaled orthographic (weak-perspective) projection.  points3D (B, N, 3), cam_params (B, 3) =
    (scale, trans x, trans y) -> (B, N, 2)."""
    return cam_params[:, None, 0:1] * (points3D[:, :, :2] + cam_params[:, None, 1:])


def perspective_project_torch(points, rotation, translation, cam_K=None, focal_length=None, img_wh=None):
    """utils/cam_utils.py:30-61: points (B, N, 3) rotated (rotation (B, 3, 3) or None), translated (B, 3), divided by depth and mapped
    by the intrinsics -- cam_K (B, 3, 3), or the matrix of utils/cam_utils.py:19-27 from ``focal_length`` and a principal point at
    img_wh / 2 -> (B, N, 2) pixels.  The training step projects its target joints with it (train_poseMF_shapeGaussian_net.py:175)."""
    from . import _capi
    _capi.require_device(points, "points")
    if cam_K is None:
        cam_K = torch.tensor([[focal_length, 0.0, img_wh / 2.0], [0.0, focal_length, img_wh / 2.0], [0.0, 0.0, 1.0]],
                             device=points.device, dtype=torch.float32).expand(points.shape[0], 3, 3)
    if rotation is not None:
        points = torch.einsum('bij,bkj->bki', rotation, points)
    points = points + translation.unsqueeze(1)
    projected = points / points[:, :, -1].unsqueeze(-1)
    return torch.einsum('bij,bkj->bki', cam_K, projected)[:, :, :-1]


def flip_about_x(points):
    """The 180 degree rotation about the x axis the training step applies to the predicted joints before projecting them
    (train/train_poseMF_shapeGaussian_net.py:276-282, 310-315; the reference goes through pytorch3d's axis-angle rotation): the exact
    diag(1, -1, -1), as sampling_utils.joints2D_error_sorted_verts_sampling uses it.  points (..., 3)."""
    return points * torch.tensor([1.0, -1.0, -1.0], device=points.device, dtype=points.dtype)
