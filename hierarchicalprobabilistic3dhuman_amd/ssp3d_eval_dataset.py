"""data/ssp3d_eval_dataset.py with the pixel work moved to the device (data_layer.py, csrc/data_layer.hip).

Same constructor and files as the reference: ``ssp3d_dir_path`` holds images/, silhouettes/ and labels.npz ('fnames', 'shapes',
'poses', 'joints2D' (n,17,3), 'bbox_centres' (n,2) as (vertical, horizontal), 'bbox_whs' (n,), 'genders').  ``__getitem__`` decodes
the image and its silhouette and returns them with the label rows; ``prepare_batch`` crops both to the bounding box with
cv2.warpAffine's arithmetic, moves the key points through the same matrix in float64 and draws the heat maps, all on the device.
The labels are taken as float64 (what the reference's arithmetic gives with float64 label arrays).  ``decode="device"`` (default
"host": nothing changes) leaves the JPEG decoding of the images to ``prepare_batch`` too (data_layer.encode_or_decode_rgb,
jpeg.DeviceJpegDecoder: the same bytes); the silhouettes stay with the host.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import data_layer


class SSP3DEvalDataset(Dataset):
    def __init__(self, ssp3d_dir_path, config, visible_joints_threshold=None, decode="host"):
        super(SSP3DEvalDataset, self).__init__()
        self.images_dir = os.path.join(ssp3d_dir_path, 'images')
        self.silhouettes_dir = os.path.join(ssp3d_dir_path, 'silhouettes')

        data = np.load(os.path.join(ssp3d_dir_path, 'labels.npz'))
        self.frame_fnames = data['fnames']
        self.body_shapes = data['shapes']
        self.body_poses = data['poses']
        self.keypoints = data['joints2D']
        self.bbox_centres = data['bbox_centres']  # Tight bounding box centre
        self.bbox_whs = data['bbox_whs']  # Tight bounding box width/height
        self.genders = data['genders']

        self.img_wh = config.DATA.PROXY_REP_SIZE
        self.hmaps_gaussian_std = config.DATA.HEATMAP_GAUSSIAN_STD
        self.bbox_scale_factor = config.DATA.BBOX_SCALE_FACTOR
        self.visible_joints_threshold = visible_joints_threshold
        self.decode = data_layer.check_decode_arg(decode)
        self._staging = self._images = None

    def __getstate__(self):                      # a worker process gets the host data only
        state = dict(self.__dict__)
        state['_staging'] = state['_images'] = None
        return state

    def __len__(self):
        return len(self.frame_fnames)

    def __getitem__(self, index):
        """{'image': (H,W,3) uint8, 'silhouette': (H,W) uint8, 'keypoints': (17,3) float64, 'bbox_centre': (2,) float64, 'bbox_wh':
        float, 'shape', 'pose': float32, 'fname', 'gender': str}."""
        if torch.is_tensor(index):
            index = index.tolist()
        fname = str(self.frame_fnames[index])
        return {'image': (data_layer.decode_rgb if self.decode == "host" else data_layer.encode_or_decode_rgb)(os.path.join(self.images_dir, fname)),
                'silhouette': data_layer.decode_grey(os.path.join(self.silhouettes_dir, fname)),
                'keypoints': torch.from_numpy(np.array(self.keypoints[index], dtype=np.float64)),
                'bbox_centre': torch.from_numpy(np.array(self.bbox_centres[index], dtype=np.float64)),
                'bbox_wh': float(self.bbox_whs[index]),
                'shape': torch.from_numpy(np.array(self.body_shapes[index])).float(),
                'pose': torch.from_numpy(np.array(self.body_poses[index])).float(),
                'fname': fname,
                'gender': str(self.genders[index])}

    def check_decoded(self):
        """decode="device": raise HpsError naming the files of the batches prepared so far whose JPEG stream was corrupt or truncated
        (their pixels are unspecified).  ``prepare_batch`` only looks at batches that have already finished; this waits for all of
        them, so call it where the host waits anyway -- the training and evaluation loops do, at the epoch's read-back and at the end."""
        if self._images is not None:
            self._images.check()

    def prepare_batch(self, items):
        """-> {'image' (B,3,wh,wh), 'heatmaps' (B,17,wh,wh), 'shape', 'pose', 'silhouette' (B,wh,wh): float32; 'keypoints' (B,17,2)
        float64; 'fname', 'gender': lists} on the current device."""
        data_layer.require_gpu("SSP3DEvalDataset.prepare_batch")
        if self._staging is None:
            self._staging = data_layer.BatchStaging()
        if self._images is None:
            self._images = data_layer.DeviceImages()
        B, np_ = len(items), data_layer.as_numpy
        images = [it['image'] for it in items]
        labels = [np.stack([np_(it[k]) for it in items]) for k in ('keypoints', 'pose', 'shape')]
        host = self._images.host_arrays(images)
        staged = self._staging.upload(labels + host + [np_(it['silhouette']) for it in items])
        keypoints, pose, shape = staged[:3]
        rgb = self._images.resolve(images, staged[3:3 + len(host)])
        boxes = [(float(it['bbox_centre'][0]), float(it['bbox_centre'][1]), it['bbox_wh']) for it in items]
        crop = data_layer.eval_crop_u8(rgb, boxes, self.bbox_scale_factor, self.img_wh, segs=staged[3 + len(host):3 + len(host) + B],
                                       keypoints=keypoints)
        heatmaps = data_layer.eval_heatmaps(crop['positions'], self.img_wh, self.hmaps_gaussian_std, keypoints=keypoints,
                                            threshold=self.visible_joints_threshold)
        return {'image': crop['rgb'], 'heatmaps': heatmaps, 'shape': shape.clone(), 'pose': pose.clone(), 'silhouette': crop['seg'],
                'keypoints': crop['joints'], 'fname': [it['fname'] for it in items], 'gender': [it['gender'] for it in items]}
