"""Camera helpers with the call surface of the reference's utils/cam_utils.py that a training step needs.  Plain tensor operations on
the device (glue between the SMPL joints and the 2D-joint loss, a few thousand numbers; autograd differentiates them as they are)."""
import torch


def orthographic_project_torch(points3D, cam_params):
    """utils/cam_utils.py:9-16: scaled orthographic (weak-perspective) projection.  points3D (B, N, 3), cam_params (B, 3) =
    (scale, trans x, trans y) -> (B, N, 2)."""
    return cam_params[:, None, 0:1] * (points3D[:, :, :2] + cam_params[:, None, 1:])


def flip_about_x(points):
    """The 180 degree rotation about the x axis the training step applies to the predicted joints before projecting them
    (train/train_poseMF_shapeGaussian_net.py:276-282, 310-315; the reference goes through pytorch3d's axis-angle rotation): the exact
    diag(1, -1, -1), as sampling_utils.joints2D_error_sorted_verts_sampling uses it.  points (..., 3)."""
    return points * torch.tensor([1.0, -1.0, -1.0], device=points.device, dtype=points.dtype)
