"""data/on_the_fly_smpl_train_dataset.py with the pixel work moved to the device (data_layer.py, csrc/data_layer.hip).

Same constructor, files (``poses_path``: npz with 'fnames' and 'poses'; ``textures_path``: npz with 'grey' and 'nongrey'
(n, 1200, 800, 3) uint8; ``backgrounds_dir_path``: a directory of .jpg files), ``__len__`` and ``params_from`` filtering as the
reference.  ``__getitem__`` makes the reference's random draws in the reference's order (:72-76, :86: torch.rand(1), one torch.randint
for the texture, one for the background -- after the same torch.manual_seed the choices are the reference's) and decodes the background;
it converts nothing to float.  ``prepare_batch`` turns a list of items into the reference's batch on the device: textures gathered from
uint8 banks that are uploaded once, backgrounds resized by cv2.resize's arithmetic, both as float32 in [0, 1].
``decode="device"`` (default "host": nothing changes) leaves the JPEG decoding to ``prepare_batch`` too: ``__getitem__`` returns the
file's bytes (data_layer.encode_or_decode_rgb) and the batch's files are decoded in one call on the device, to the same bytes.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import data_layer


class OnTheFlySMPLTrainDataset(Dataset):
    def __init__(self, poses_path, textures_path, backgrounds_dir_path, params_from='all', grey_tex_prob=0.05, img_wh=256, decode="host"):
        assert params_from in ['all', 'h36m', 'up3d', '3dpw', 'amass', 'not_amass']
        data = np.load(poses_path)
        fnames, poses = data['fnames'], data['poses']
        if params_from != 'all':
            real = lambda x: x.startswith('h36m') or x.startswith('up3d') or x.startswith('3dpw')
            if params_from == 'not_amass':
                keep = [i for i, x in enumerate(fnames) if real(x)]
            elif params_from == 'amass':
                keep = [i for i, x in enumerate(fnames) if not real(x)]
            else:
                keep = [i for i, x in enumerate(fnames) if x.startswith(params_from)]
            fnames, poses = [fnames[i] for i in keep], [poses[i] for i in keep]
        self.fnames = fnames
        self.poses = np.stack(poses, axis=0) if len(poses) else np.zeros((0, 72), dtype=np.float32)

        textures = np.load(textures_path)
        self.grey_textures = textures['grey']
        self.nongrey_textures = textures['nongrey']
        for bank in (self.grey_textures, self.nongrey_textures):
            assert bank.dtype == np.uint8 and (len(bank) == 0 or bank.shape[-3:] == (1200, 800, 3)), \
                "Texture shape is wrong: {}".format(bank.shape)
        self.grey_tex_prob = grey_tex_prob

        self.backgrounds_paths = sorted([os.path.join(backgrounds_dir_path, f) for f in os.listdir(backgrounds_dir_path)
                                         if f.endswith('.jpg')])
        self.img_wh = img_wh
        self.decode = data_layer.check_decode_arg(decode)
        self._banks = self._staging = self._images = None

    def __getstate__(self):                      # a worker process gets the host data only
        state = dict(self.__dict__)
        state['_banks'] = state['_staging'] = state['_images'] = None
        return state

    def __len__(self):
        return len(self.poses)

    def __getitem__(self, index):
        """{'pose': (72,) float32, 'texture_choice': (is_grey, tex_idx), 'background': (H, W, 3) uint8 of the file's own size}; under
        decode="device" the background is a jpeg.EncodedJpeg where the device can decode the file."""
        if torch.is_tensor(index):
            index = index.tolist()
        if isinstance(index, (list, tuple)):
            raise TypeError("OnTheFlySMPLTrainDataset takes one index per item; batches are formed by prepare_batch")
        pose = torch.from_numpy(self.poses[index].astype(np.float32))
        is_grey = torch.rand(1).item() < self.grey_tex_prob
        bank = self.grey_textures if is_grey else self.nongrey_textures
        tex_idx = torch.randint(low=0, high=len(bank), size=(1,)).item()
        bg_idx = torch.randint(low=0, high=len(self.backgrounds_paths), size=(1,)).item()
        return {'pose': pose, 'texture_choice': (bool(is_grey), int(tex_idx)),
                'background': (data_layer.decode_rgb if self.decode == "host" else data_layer.encode_or_decode_rgb)(self.backgrounds_paths[bg_idx])}

    def check_decoded(self):
        """decode="device": raise HpsError naming the files of the batches prepared so far whose JPEG stream was corrupt or truncated
        (their pixels are unspecified).  ``prepare_batch`` only looks at batches that have already finished; this waits for all of
        them, so call it where the host waits anyway -- the training and evaluation loops do, at the epoch's read-back and at the end."""
        if self._images is not None:
            self._images.check()

    def prepare_batch(self, items):
        """-> {'pose': (B,72), 'texture': (B,1200,800,3), 'background': (B,3,img_wh,img_wh)}, float32 on the current device."""
        data_layer.require_gpu("OnTheFlySMPLTrainDataset.prepare_batch")
        dev = data_layer.current_device()
        if self._banks is None or self._banks[0].device != dev:
            self._banks = (torch.from_numpy(np.ascontiguousarray(self.grey_textures)).to(dev),
                           torch.from_numpy(np.ascontiguousarray(self.nongrey_textures)).to(dev))
            self._staging = data_layer.BatchStaging()
        if self._images is None:
            self._images = data_layer.DeviceImages()
        poses = np.stack([data_layer.as_numpy(it['pose']) for it in items]).astype(np.float32, copy=False)
        backgrounds = [it['background'] for it in items]
        staged = self._staging.upload([poses] + self._images.host_arrays(backgrounds))
        texture = data_layer.texture_gather(self._banks[0], self._banks[1], [it['texture_choice'] for it in items])
        background = data_layer.resize_bilinear_u8(self._images.resolve(backgrounds, staged[1:]), (self.img_wh, self.img_wh))
        return {'pose': staged[0].clone(), 'texture': texture, 'background': background}
