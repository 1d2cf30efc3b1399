"""train/train_poseMF_shapeGaussian_net.py on the device: one synthetic-data training / validation step (``SyntheticTrainStep``) and the
epoch loop with the reference's signature and return value (``train_poseMF_shapeGaussian_net``).

Every part of the step is a device component of this package -- the renderer (textured_renderer.TexturedIUVRenderer), the crop /
augment / visibility front end (train_augmentation.SyntheticTrainFrontEnd), the differentiable encoder, head, sampler and SMPL, the
loss (matrix_fisher_loss.PoseMFShapeGaussianLoss), the optimiser (device_optim.DeviceAdam) and the loss-and-metrics tracker
(train_loss_and_metrics_tracker, one library call per step).  The step makes no host synchronisation of its own: the host draws its
random numbers in the reference's order, uploads them, and queues launches; the tracker is read back once per epoch.

Two differences that this code base forces:

* ``pose_shape_model.train()`` is refused by the encoder unless ``set_batchnorm_training(True)`` opted in to batch statistics
  (resnet.py).  The loop opts in itself -- and to ``set_differentiable_factors(True)``, which the stage-2 samples need and which
  changes no launch and no bit of the forward -- and restores both settings on exit.  Any torch optimiser works, but only
  ``DeviceAdam(..., refresh=(pose_shape_model,))`` keeps the model's derived device state (permuted / folded weights, launch lists)
  alive behind a step; behind any other optimiser the model notices the step and rebuilds that state at its next forward.  The
  loop itself drops the derived state once, at the start of every epoch, so that an epoch resumed from a checkpoint repeats the
  uninterrupted one bit for bit.
* ``train_dataset`` / ``val_dataset`` are whatever yields the reference's item dict: 'pose' (72,) axis-angle, 'background'
  (3, img_wh, img_wh), 'texture' (Ht, Wt, 3) -- or a dataset with ``prepare_batch`` (on_the_fly_smpl_train_dataset.py): its raw items
  pass through the DataLoader as they are and each list of them becomes the batch on the device (data_layer.py).
"""
import copy
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import cam_utils, data_layer, rigid_transform_utils as rtu, sampling_utils, textured_renderer, train_augmentation
from .checkpoint_utils import load_training_info_from_checkpoint
from .device_state import DeviceStateModule
from .label_conversions import ALL_JOINTS_TO_COCO_MAP, ALL_JOINTS_TO_H36M_MAP, H36M_TO_J14
from .train_loss_and_metrics_tracker import TrainingLossesAndMetricsTracker

_J14 = [ALL_JOINTS_TO_H36M_MAP[i] for i in H36M_TO_J14]                      # :156-157 / :274-275 in one gather


class SyntheticTrainStep:
    """One iteration of the reference's batch loop (:119-370).  Built once per training run: the pre-defined tensors of :83-91, the
    renderer, the front end and the tracker live here; ``step(samples_batch, split)`` runs data generation (:123-256), the forward
    (:258-322), the loss and -- for 'train' -- the backward and the optimiser step (:327-349), and the tracker's update (:354-370,
    with the loss as a device tensor and the front end's status words).  Returns the loss, a 0-dim device tensor.

    ``last`` holds the step's dicts (what the loss and the tracker saw) for whoever wants to look; the front end's buffers in it are
    overwritten by the next step."""

    def __init__(self, pose_shape_model, pose_shape_cfg, smpl_model, edge_detect_model, pytorch3d_renderer, device, criterion,
                 optimiser, metrics_tracker):
        cfg = pose_shape_cfg
        self.model, self.cfg, self.smpl, self.renderer = pose_shape_model, cfg, smpl_model, pytorch3d_renderer
        self.device, self.criterion, self.optimiser, self.tracker = torch.device(device), criterion, optimiser, metrics_tracker
        B, f32 = cfg.TRAIN.BATCH_SIZE, dict(device=self.device, dtype=torch.float32)
        # :83-91
        self.delta_betas_std_vector = torch.ones(cfg.MODEL.NUM_SMPL_BETAS, **f32) * cfg.TRAIN.SYNTH_DATA.AUGMENT.SMPL.SHAPE_STD
        self.mean_shape = torch.zeros(cfg.MODEL.NUM_SMPL_BETAS, **f32)
        self.mean_cam_t = torch.tensor(cfg.TRAIN.SYNTH_DATA.MEAN_CAM_T, **f32)[None, :].expand(B, -1)
        self.zero_pose = torch.zeros(B, 72, **f32)                            # the reposed meshes' pose (:159-160, :287-288)
        self.front_end = train_augmentation.SyntheticTrainFrontEnd(
            cfg.TRAIN.SYNTH_DATA.AUGMENT, cfg.DATA.PROXY_REP_SIZE, edge_detect_model, cfg.DATA.HEATMAP_GAUSSIAN_STD, cfg.DATA.EDGE_NMS,
            bbox_scale_factor=cfg.DATA.BBOX_SCALE_FACTOR)
        self.last = None

    def _project(self, joints_all, cam_wp):
        """:276-284 / :310-317: the COCO joints, turned by pi about x, under the predicted weak-perspective camera."""
        return cam_utils.orthographic_project_torch(cam_utils.flip_about_x(joints_all[:, ALL_JOINTS_TO_COCO_MAP, :]), cam_wp)

    def generate(self, samples_batch):
        """:123-256 under no_grad -> (proxy_rep_input, target dict, target_reposed_vertices).  The host draws, in the reference's
        order: the shape (:141), the camera (:145), the light (:186), then the front end's plan (:199-244)."""
        cfg, dev = self.cfg, self.device
        B, synth, wh = cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.SYNTH_DATA, cfg.DATA.PROXY_REP_SIZE
        with torch.no_grad():
            target_pose = samples_batch['pose'].to(dev)
            background = samples_batch['background'].to(dev)
            texture = samples_batch['texture'].to(dev)
            rotmats = rtu.batch_rodrigues(target_pose.contiguous().view(-1, 3)).view(-1, 24, 3, 3)
            # :136-139, rot_mult_order 'post': R diag(1, -1, -1) -- the second and third COLUMNS change sign
            target_glob_rotmats = cam_utils.flip_about_x(rotmats[:, 0, :, :])
            target_pose_rotmats = rotmats[:, 1:, :, :]
            target_shape = textured_renderer.normal_sample_shape(B, self.mean_shape, self.delta_betas_std_vector)
            target_cam_t = textured_renderer.augment_cam_t(self.mean_cam_t, xy_std=synth.AUGMENT.CAM.XY_STD,
                                                           delta_z_range=synth.AUGMENT.CAM.DELTA_Z_RANGE)
            target_out = self.smpl(body_pose=target_pose_rotmats, global_orient=target_glob_rotmats.unsqueeze(1), betas=target_shape,
                                   pose2rot=False)
            target_vertices, target_joints_all = target_out.vertices, target_out.joints
            target_reposed_vertices = self.smpl(body_pose=self.zero_pose[:, 3:], global_orient=self.zero_pose[:, :3],
                                                betas=target_shape).vertices
            # :167-179: turned the right way up for the camera
            joints2d = cam_utils.perspective_project_torch(cam_utils.flip_about_x(target_joints_all[:, ALL_JOINTS_TO_COCO_MAP, :]), None,
                                                           target_cam_t, focal_length=synth.FOCAL_LENGTH, img_wh=wh)
            lights = textured_renderer.augment_light(batch_size=1, device=dev, rgb_augment_config=synth.AUGMENT.RGB)
            iuv_in, rgb_in = self.renderer.render_train_inputs(vertices=cam_utils.flip_about_x(target_vertices), textures=texture,
                                                               cam_t=target_cam_t, lights_rgb_settings=lights)
            plan = train_augmentation.draw_augment_plan(synth.AUGMENT, B, wh)
            front = self.front_end(iuv_in, rgb_in, background, joints2d.contiguous(), plan=plan)
        target = {'pose_params_rotmats': target_pose_rotmats, 'shape_params': target_shape, 'verts': target_vertices,
                  'joints3D': target_joints_all[:, _J14, :], 'joints2D': front['joints2D'], 'joints2D_vis': front['joints2D_vis'],
                  'glob_rotmats': target_glob_rotmats}
        return front['proxy_rep_input'], target, target_reposed_vertices

    def forward(self, proxy_rep_input):
        """:262-322 -> (pred dict for the loss, pred_joints2d_coco_mode, pred_reposed_vertices_mean)."""
        cfg = self.cfg
        N = cfg.LOSS.NUM_SAMPLES
        pose_F, pose_U, pose_S, pose_V, rotmats_mode, shape_dist, glob, cam_wp = self.model(proxy_rep_input)
        glob_rotmats = rtu.rot6d_to_rotmat(glob)
        mode_out = self.smpl(body_pose=rotmats_mode, global_orient=glob_rotmats.unsqueeze(1), betas=shape_dist.loc, pose2rot=False)
        joints2d_mode = self._project(mode_out.joints, cam_wp)
        with torch.no_grad():
            reposed = self.smpl(body_pose=self.zero_pose[:, 3:], global_orient=self.zero_pose[:, :3], betas=shape_dist.loc).vertices
        j2d_loss_on = self.criterion.loss_config.J2D_LOSS_ON
        if 'samples' in j2d_loss_on:
            rotmats_samples = sampling_utils.pose_matrix_fisher_sampling_torch(pose_U=pose_U, pose_S=pose_S, pose_V=pose_V, num_samples=N,
                                                                               b=1.5, oversampling_ratio=8,
                                                                               sample_on_cpu=cfg.LOSS.SAMPLE_ON_CPU)
            shape_samples = shape_dist.rsample([N]).transpose(0, 1)                                       # (bs, N, betas)
            joints_samples = self.smpl(body_pose=rotmats_samples.reshape(-1, 23, 3, 3),
                                       global_orient=glob_rotmats[:, None, :, :].expand(-1, N, -1, -1).reshape(-1, 1, 3, 3),
                                       betas=shape_samples.reshape(-1, shape_samples.shape[-1]), pose2rot=False).joints
            joints2d_samples = self._project(joints_samples, cam_wp[:, None, :].expand(-1, N, -1).reshape(-1, 3))
            joints2d_samples = joints2d_samples.reshape(-1, N, joints2d_samples.shape[1], 2)
            if j2d_loss_on == 'means+samples':
                joints2d_samples = torch.cat([joints2d_mode[:, None, :, :], joints2d_samples], dim=1)
        else:
            joints2d_samples = joints2d_mode[:, None, :, :]
        pred = {'pose_params_F': pose_F, 'pose_params_U': pose_U, 'pose_params_S': pose_S, 'pose_params_V': pose_V,
                'shape_params': shape_dist, 'verts': mode_out.vertices, 'joints3D': mode_out.joints[:, _J14, :],
                'joints2D': joints2d_samples, 'glob_rotmats': glob_rotmats}
        return pred, joints2d_mode, reposed

    def __call__(self, samples_batch, split):
        assert split in ('train', 'val')
        proxy_rep_input, target, target_reposed = self.generate(samples_batch)
        with torch.set_grad_enabled(split == 'train'):
            pred, joints2d_mode, pred_reposed = self.forward(proxy_rep_input)
            self.optimiser.zero_grad()
            loss = self.criterion(target, pred)
            if split == 'train':
                loss.backward()
                self.optimiser.step()
        # :354-363: what the tracker looks at
        j2d_loss_on = self.criterion.loss_config.J2D_LOSS_ON
        tracked = {'verts': pred['verts'], 'joints3D': pred['joints3D'], 'joints2D': joints2d_mode}
        if j2d_loss_on == 'samples':
            tracked['joints2Dsamples'] = pred['joints2D']
        elif j2d_loss_on == 'means+samples':
            tracked['joints2Dsamples'] = pred['joints2D'][:, 1:, :, :]
        self.tracker.update_per_batch(split=split, loss=loss, pred_dict=tracked, target_dict=target,
                                      batch_size=self.cfg.TRAIN.BATCH_SIZE, pred_reposed_vertices=pred_reposed,
                                      target_reposed_vertices=target_reposed, status=self.front_end.status())
        self.last = dict(pred=pred, target=target, tracked=tracked, pred_reposed=pred_reposed, target_reposed=target_reposed)
        return loss.detach()


def _progress(iterable):
    """tqdm's bar where tqdm is installed (the reference imports it unconditionally), the bare iterable elsewhere."""
    try:
        from tqdm import tqdm
    except ImportError:
        return iterable
    return tqdm(iterable)


def train_poseMF_shapeGaussian_net(pose_shape_model,
                                   pose_shape_cfg,
                                   smpl_model,
                                   edge_detect_model,
                                   pytorch3d_renderer,
                                   device,
                                   train_dataset,
                                   val_dataset,
                                   criterion,
                                   optimiser,
                                   metrics,
                                   model_save_dir,
                                   logs_save_path,
                                   save_val_metrics=['PVE-SC', 'MPJPE-PA'],
                                   checkpoint=None):
    """train/train_poseMF_shapeGaussian_net.py:27-405 with the same arguments and return value (``pose_shape_model`` holding the best
    epoch's weights).  ``pytorch3d_renderer``: a textured_renderer.TexturedIUVRenderer with render_rgb=True; ``edge_detect_model``: a
    canny_edge_detector.CannyEdgeDetector; ``metrics``: the list of metric names, to which 'joints2Dsamples-L2E' is appended at the
    stage change as the reference appends it.  As there, the caller loads the model's and the optimiser's state dicts from
    ``checkpoint`` before the call.  The module docstring has the two differences (BatchNorm opt-in, datasets)."""
    cfg = pose_shape_cfg
    if getattr(pose_shape_model.image_encoder, "_forward_only", False):          # before a file, a loader or a buffer is touched
        raise NotImplementedError("training a net with the Bottleneck (ResNet-50) encoder is not implemented: its encoder runs forward "
                                  "only (MODEL.NUM_RESNET_LAYERS = 18 trains; so does 50 after set_differentiable_encoder(True))")
    def loader(dataset):
        # a dataset with prepare_batch (on_the_fly_smpl_train_dataset.py) hands over raw items: its batch is formed on the device
        raw = data_layer.preparer(dataset) is not None
        return DataLoader(dataset, batch_size=cfg.TRAIN.BATCH_SIZE, shuffle=True, drop_last=True, num_workers=cfg.TRAIN.NUM_WORKERS,
                          pin_memory=False if raw else cfg.TRAIN.PIN_MEMORY, collate_fn=data_layer.passthrough_collate if raw else None)
    dataloaders = {'train': loader(train_dataset), 'val': loader(val_dataset)}
    prepare = {'train': data_layer.preparer(train_dataset), 'val': data_layer.preparer(val_dataset)}

    if checkpoint is not None:
        current_epoch, best_epoch, best_model_wts, best_epoch_val_metrics = load_training_info_from_checkpoint(checkpoint, save_val_metrics)
        load_logs = True
    else:
        current_epoch, best_epoch = 0, 0
        best_epoch_val_metrics = {metric: np.inf for metric in save_val_metrics}
        best_model_wts = copy.deepcopy(pose_shape_model.state_dict())
        load_logs = False

    metrics_tracker = TrainingLossesAndMetricsTracker(metrics_to_track=metrics, img_wh=cfg.DATA.PROXY_REP_SIZE, log_save_path=logs_save_path,
                                                      load_logs=load_logs, current_epoch=current_epoch)
    step = SyntheticTrainStep(pose_shape_model, cfg, smpl_model, edge_detect_model, pytorch3d_renderer, device, criterion, optimiser,
                              metrics_tracker)

    previous = (pose_shape_model.image_encoder._bn_training, pose_shape_model.differentiable_factors)
    pose_shape_model.set_batchnorm_training(True)
    pose_shape_model.set_differentiable_factors(True)
    try:
        current_loss_stage = 1
        for epoch in range(current_epoch, cfg.TRAIN.NUM_EPOCHS):
            print('\nEpoch {}/{}'.format(epoch, cfg.TRAIN.NUM_EPOCHS - 1))
            print('-' * 10)
            metrics_tracker.initialise_loss_metric_sums()
            # An epoch starts from device state built from the parameters alone, as a run resumed from this epoch's checkpoint starts:
            # the in-place refresh behind an optimiser step may leave the Winograd stem's weights one unit in the last place from a
            # fresh build (device_optim; tests/optim_scenario.compare_states).  One rebuild per epoch; within the epoch nothing moves.
            for module in pose_shape_model.modules():
                if isinstance(module, DeviceStateModule):
                    module.invalidate()

            if epoch >= cfg.LOSS.STAGE_CHANGE_EPOCH and current_loss_stage == 1:
                # 2D samples losses + 3D mode losses + the stage's weighting from this epoch onwards
                criterion.loss_config = cfg.LOSS.STAGE2
                print('Stage 2 loss config:\n', criterion.loss_config)
                print('Sample on CPU:', cfg.LOSS.SAMPLE_ON_CPU)
                metrics_tracker.metrics_to_track.append('joints2Dsamples-L2E')
                print('Tracking metrics:', metrics_tracker.metrics_to_track)
                current_loss_stage = 2

            for split in ['train', 'val']:
                if split == 'train':
                    print('Training.')
                    pose_shape_model.train()
                else:
                    print('Validation.')
                    pose_shape_model.eval()
                for samples_batch in _progress(dataloaders[split]):
                    if prepare[split] is not None:
                        samples_batch = prepare[split](samples_batch)
                    step(samples_batch, split)

            metrics_tracker.update_per_epoch()                  # the epoch's one read-back; raises for an image that had no body pixel
            sampling_utils.check_sampling()
            for checked in (train_dataset, val_dataset):        # decode="device": corrupt or truncated JPEG files of the epoch, by name
                data_layer.check_decoded(checked)

            if metrics_tracker.determine_save_model_weights_this_epoch(save_val_metrics, best_epoch_val_metrics):
                for metric in save_val_metrics:
                    best_epoch_val_metrics[metric] = metrics_tracker.epochs_history['val_' + metric][-1]
                print("Best epoch val metrics updated to ", best_epoch_val_metrics)
                best_model_wts = copy.deepcopy(pose_shape_model.state_dict())
                best_epoch = epoch
                print("Best model weights updated!")

            if epoch % cfg.TRAIN.EPOCHS_PER_SAVE == 0:
                save_dict = {'epoch': epoch,
                             'best_epoch': best_epoch,
                             'best_epoch_val_metrics': best_epoch_val_metrics,
                             'model_state_dict': pose_shape_model.state_dict(),
                             'best_model_state_dict': best_model_wts,
                             'optimiser_state_dict': optimiser.state_dict()}
                torch.save(save_dict, os.path.join(model_save_dir, 'epoch_{}'.format(str(epoch).zfill(3)) + '.tar'))
                print('Model saved! Best Val Metrics:\n', best_epoch_val_metrics, '\nin epoch {}'.format(best_epoch))

        print('Training Completed. Best Val Metrics:\n', best_epoch_val_metrics)
    finally:
        pose_shape_model.set_batchnorm_training(previous[0])
        pose_shape_model.set_differentiable_factors(previous[1])

    pose_shape_model.load_state_dict(best_model_wts)
    return pose_shape_model
