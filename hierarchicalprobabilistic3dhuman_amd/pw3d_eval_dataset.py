"""data/pw3d_eval_dataset.py with the pixel work moved to the device (data_layer.py, csrc/data_layer.hip).

Same constructor and files as the reference: ``pw3d_dir_path`` holds cropped_frames/, 3dpw_test.npz ('imgname', 'pose', 'shape',
'gender') and hrnet_results_centred.npy (n,17,3).  ``__getitem__`` decodes the cropped frame (square, else the reference's assertion);
``prepare_batch`` resizes with cv2.resize's arithmetic, scales the key points in float64, rounds them half to even and draws the heat
maps, all on the device.  ``decode="device"`` (default "host": nothing changes) leaves the JPEG decoding to ``prepare_batch`` too
(data_layer.encode_or_decode_rgb, jpeg.DeviceJpegDecoder): the same bytes, decoded per batch on the device.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import data_layer


class PW3DEvalDataset(Dataset):
    def __init__(self, pw3d_dir_path, config, visible_joints_threshold=None, decode="host"):
        super(PW3DEvalDataset, self).__init__()
        self.cropped_frames_dir = os.path.join(pw3d_dir_path, 'cropped_frames')

        data = np.load(os.path.join(pw3d_dir_path, '3dpw_test.npz'))
        self.frame_fnames = data['imgname']
        self.pose = data['pose']
        self.shape = data['shape']
        self.gender = data['gender']

        self.keypoints = np.load(os.path.join(pw3d_dir_path, 'hrnet_results_centred.npy'))

        self.img_wh = config.DATA.PROXY_REP_SIZE
        self.hmaps_gaussian_std = config.DATA.HEATMAP_GAUSSIAN_STD
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
        """{'image': (S,S,3) uint8, 'keypoints': (17,3) float64, 'pose', 'shape': float32, 'fname', 'gender': str}."""
        if torch.is_tensor(index):
            index = index.tolist()
        fname = str(self.frame_fnames[index])
        image = (data_layer.decode_rgb if self.decode == "host" else data_layer.encode_or_decode_rgb)(os.path.join(self.cropped_frames_dir, fname))
        orig_height, orig_width = image.shape[:2]
        assert (orig_height == orig_width), "Resizing non-square image to square will cause unwanted stretching/squeezing!"
        return {'image': image,
                'keypoints': torch.from_numpy(np.array(self.keypoints[index], dtype=np.float64)),
                'pose': torch.from_numpy(np.array(self.pose[index])).float(),
                'shape': torch.from_numpy(np.array(self.shape[index])).float(),
                'fname': fname,
                'gender': str(self.gender[index])}

    def check_decoded(self):
        """decode="device": raise HpsError naming the files of the batches prepared so far whose JPEG stream was corrupt or truncated
        (their pixels are unspecified).  ``prepare_batch`` only looks at batches that have already finished; this waits for all of
        them, so call it where the host waits anyway -- the training and evaluation loops do, at the epoch's read-back and at the end."""
        if self._images is not None:
            self._images.check()

    def prepare_batch(self, items):
        """-> {'image' (B,3,wh,wh), 'heatmaps' (B,17,wh,wh), 'pose', 'shape': float32; 'fname', 'gender': lists} on the current device."""
        data_layer.require_gpu("PW3DEvalDataset.prepare_batch")
        if self._staging is None:
            self._staging = data_layer.BatchStaging()
        if self._images is None:
            self._images = data_layer.DeviceImages()
        np_, wh = data_layer.as_numpy, self.img_wh
        images = [it['image'] for it in items]
        labels = [np.stack([np_(it[k]) for it in items]) for k in ('keypoints', 'pose', 'shape')]
        # :51-52: img_wh / float(orig_width), img_wh / float(orig_height) -- Python floats
        scale = np.array([[wh / float(it['image'].shape[1]), wh / float(it['image'].shape[0])] for it in items], dtype=np.float64)
        staged = self._staging.upload(labels + [scale] + self._images.host_arrays(images))
        keypoints, pose, shape, scale_d = staged[:4]
        image = data_layer.resize_bilinear_u8(self._images.resolve(images, staged[4:]), (wh, wh))
        _, positions = data_layer.keypoints_scale_round(keypoints, scale_d)
        heatmaps = data_layer.eval_heatmaps(positions, wh, self.hmaps_gaussian_std, keypoints=keypoints,
                                            threshold=self.visible_joints_threshold)
        return {'image': image, 'heatmaps': heatmaps, 'pose': pose.clone(), 'shape': shape.clone(),
                'fname': [it['fname'] for it in items], 'gender': [it['gender'] for it in items]}
