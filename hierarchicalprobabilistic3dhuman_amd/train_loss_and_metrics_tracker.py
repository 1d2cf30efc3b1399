"""metrics/train_loss_and_metrics_tracker.py on the device.

The reference's tracker copies the predicted and target vertices, reposed vertices and joints to the host every step, calls
``loss.item()`` (which drains the stream), runs numpy Procrustes and adds the results into Python sums.  Here ``update_per_batch`` is
ONE library call (include/hps.h: hps_train_metrics_update, csrc/metrics.hip): the batch's metrics are formed on the device and added
into running sums that stay there; ``update_per_epoch`` reads them back once.  No ``.item()``, no ``.cpu()``, no torch kernel, nothing
allocated after the first call of a batch size, and the caller's dicts are left as they are (the reference replaces their tensors by
numpy arrays -- its way of converting, not a contract).

Differences from the reference, all deliberate:

* the epoch sums are float64.  The reference's are float32: ``np.sum`` of a float32 array is a float32 scalar, and numpy's
  ``float32 + python float`` stays float32, so after the first batch every ``+=`` rounds to 24 bits.  The per-point arithmetic is
  that of ``eval_utils.pointset_errors`` (float64 statistics, fp32 transform and distances, float64 sums).
* ``metrics_to_track`` is read at each call (the training loop appends ``joints2Dsamples-L2E`` at the stage change).
* the per-sample divisors of ``update_per_epoch`` come from the tensors' shapes (6890 / 14 / 17 for the reference's data).
* ``update_per_batch(..., status=front_end.status())`` counts the front end's empty-box words on the device; ``update_per_epoch``
  raises the error ``SyntheticTrainFrontEnd.check()`` would have raised -- one synchronisation per epoch instead of one per step.
"""
import ctypes
import pickle

import torch

from . import _capi

METRIC_NAMES = ('PVE', 'PVE-SC', 'PVE-PA', 'PVE-T', 'PVE-T-SC', 'MPJPE', 'MPJPE-SC', 'MPJPE-PA', 'joints2D-L2E',
                'joints2Dsamples-L2E')
METRIC_BITS = {name: 1 << i for i, name in enumerate(METRIC_NAMES)}          # include/hps.h: HPS_TRAIN_METRIC_*
NSLOT = _capi.TRAIN_METRICS_NSLOT
SLOT_LOSS, SLOT_SAMPLES, SLOT_METRIC0, SLOT_VISIBLE, SLOT_STATUS = 0, 1, 2, 12, 13
SPLITS = ('train', 'val')


def metrics_mask(metrics_to_track):
    """The HPS_TRAIN_METRIC_* bits of a list of metric names (unknown names are ignored, as the reference ignores them)."""
    mask = 0
    for name in metrics_to_track:
        mask |= METRIC_BITS.get(name, 0)
    return mask


class TrainingLossesAndMetricsTracker:
    """The reference's tracker (:8-245): the same constructor, ``all_metrics_types``, ``epochs_history`` keys and methods; what
    differs is in the module docstring."""

    def __init__(self, metrics_to_track, img_wh, log_save_path, load_logs=False, current_epoch=None):
        self.all_metrics_types = ['%s_%s' % (split, name) for name in METRIC_NAMES for split in SPLITS]         # :20-29, same order
        self.metrics_to_track = metrics_to_track             # the caller's list itself: the loop appends to it at the stage change
        self.img_wh = img_wh
        self.log_save_path = log_save_path
        if load_logs:
            self.epochs_history = self.load_history(log_save_path, current_epoch)
        else:
            self.epochs_history = {key: [] for key in ['train_losses', 'val_losses'] + self.all_metrics_types}
        self.loss_metric_sums = None
        self._sums = None                    # (2, NSLOT) float64 on the device: rows train / val
        self._ws = {}                        # number of sets -> workspace
        self._args = _capi.TrainMetricsArgs(struct_bytes=ctypes.sizeof(_capi.TrainMetricsArgs))
        self._per_sample = {'PVE': 6890, 'MPJPE': 14, 'joints2D': 17}       # replaced by the shapes update_per_batch sees

    def load_history(self, load_log_path, current_epoch):
        """:44-72: the pickled history cut to ``current_epoch`` entries per key; a metric the log lacks is filled with zeros; every
        list must then hold exactly ``current_epoch`` entries."""
        with open(load_log_path, 'rb') as f:
            history = pickle.load(f)
        for key in ['train_losses', 'val_losses'] + self.all_metrics_types:
            if key in history:
                history[key] = history[key][:current_epoch]
            else:
                history[key] = [0.0] * current_epoch
                print(key, 'filled with zeros up to epoch', current_epoch)
        for key, values in history.items():
            assert len(values) == current_epoch, "{} elements in {} list when current epoch is {}".format(len(values), key, current_epoch)
        print('Logs loaded from', load_log_path)
        return history

    def initialise_loss_metric_sums(self):
        """:74-86.  The device sums are zeroed by an asynchronous fill on the current stream (they are allocated by the first update,
        which knows the device); ``loss_metric_sums`` keeps the reference's keys and receives the sums in ``update_per_epoch``."""
        self.loss_metric_sums = {}
        for split in SPLITS:
            self.loss_metric_sums[split + '_losses'] = 0.
            self.loss_metric_sums[split + '_num_samples'] = 0
            self.loss_metric_sums[split + '_num_visib_joints2Dsamples'] = 0.
            for name in METRIC_NAMES:
                self.loss_metric_sums[split + '_' + name] = 0.
        if self._sums is not None:
            self._sums.zero_()

    def device_sums(self):
        """(2, NSLOT) float64 device tensor of the running sums (rows train / val; slots: include/hps.h), or None before the first
        update.  Reading it synchronises; the tracker itself does so only in update_per_epoch."""
        return self._sums

    def per_set_values(self, num_sets):
        """What the last update of ``num_sets`` sets left in its workspace (include/hps.h): (part (3, B, 3) float64 -- family (vertices,
        reposed vertices, joints), set, mode (raw, SC, PA) -- and j2d (B, 3) float64 -- joints2D-L2E, joints2Dsamples-L2E, visible
        joint samples), views of the workspace; entries of metrics that were not tracked are stale.  For tests and diagnosis."""
        ws, B = self._ws[num_sets], num_sets
        return ws[3 * 17 * B:(3 * 17 + 9) * B].view(3, B, 3), ws[(3 * 17 + 9) * B:(3 * 17 + 12) * B].view(B, 3)

    def update_per_batch(self,
                         split,
                         loss,
                         pred_dict,
                         target_dict,
                         batch_size,
                         pred_reposed_vertices=None,
                         target_reposed_vertices=None,
                         status=None):
        assert split in ['train', 'val'], "Invalid split in metric tracker batch update."
        if self.loss_metric_sums is None:
            raise _capi.HpsError("call initialise_loss_metric_sums() before update_per_batch()")
        tracked = self.metrics_to_track
        mask = metrics_mask(tracked)
        if any(['PVE-T' in metric_type for metric_type in tracked]):
            assert (pred_reposed_vertices is not None) and \
                   (target_reposed_vertices is not None), \
                "Need to pass reposed vertices to metric tracker batch update."

        _capi.require_device(loss, "loss")
        a = self._args
        keep = []                            # tensors that must outlive the call's launches (conversions, if any)

        def sets(t, what, last):
            """t (..., n, last) -> fp32 contiguous (-1, n, last), as the reference's reshape(-1, n, last)."""
            _capi.require_device(t, what)
            t = _capi.f32c(t.detach())
            if t.dim() < 3 or t.shape[-1] != last:
                raise _capi.HpsError("%s must be (..., n, %d), got %s" % (what, last, tuple(t.shape)))
            t = t.reshape(-1, t.shape[-2], last)
            keep.append(t)
            return t

        def pair(pred, target, what, last=3):
            p, t = sets(pred, "pred " + what, last), sets(target, "target " + what, last)
            if p.shape != t.shape:
                raise _capi.HpsError("pred and target %s differ in shape: %s, %s" % (what, tuple(p.shape), tuple(t.shape)))
            return p, t

        B = None

        def count(n, what):
            nonlocal B
            if B is None:
                B = n
            elif B != n:
                raise _capi.HpsError("%s holds %d sets, the tensors before it %d" % (what, n, B))

        for f in ("pred_verts", "target_verts", "pred_reposed", "target_reposed", "pred_joints3d", "target_joints3d", "pred_joints2d",
                  "target_joints2d", "pred_joints2d_samples", "vis", "status"):
            setattr(a, f, None)
        a.P = a.J = a.K = a.N = a.num_status = 0
        if mask & 0x7:
            p, t = pair(pred_dict['verts'], target_dict['verts'], "verts")
            count(p.shape[0], "verts")
            a.pred_verts, a.target_verts, a.P = _capi.ptr(p), _capi.ptr(t), p.shape[1]
            self._per_sample['PVE'] = p.shape[1]
        if mask & 0x18:
            p, t = pair(pred_reposed_vertices, target_reposed_vertices, "reposed vertices")
            count(p.shape[0], "reposed vertices")
            if a.P not in (0, p.shape[1]):
                raise _capi.HpsError("verts and reposed vertices differ in their number of points")
            a.pred_reposed, a.target_reposed, a.P = _capi.ptr(p), _capi.ptr(t), p.shape[1]
            self._per_sample['PVE'] = p.shape[1]
        if mask & 0xe0:
            p, t = pair(pred_dict['joints3D'], target_dict['joints3D'], "joints3D")
            count(p.shape[0], "joints3D")
            a.pred_joints3d, a.target_joints3d, a.J = _capi.ptr(p), _capi.ptr(t), p.shape[1]
            self._per_sample['MPJPE'] = p.shape[1]
        if mask & 0x300:
            t2 = sets(target_dict['joints2D'], "target joints2D", 2)
            count(t2.shape[0], "joints2D")
            a.target_joints2d, a.K = _capi.ptr(t2), t2.shape[1]
            self._per_sample['joints2D'] = t2.shape[1]
        if mask & 0x100:
            p2 = sets(pred_dict['joints2D'], "pred joints2D", 2)
            if p2.shape != t2.shape:
                raise _capi.HpsError("pred and target joints2D differ in shape: %s, %s" % (tuple(p2.shape), tuple(t2.shape)))
            a.pred_joints2d = _capi.ptr(p2)
        if mask & 0x200:
            ps = pred_dict['joints2Dsamples']
            _capi.require_device(ps, "pred joints2Dsamples")
            ps = _capi.f32c(ps.detach())
            vis = target_dict['joints2D_vis']
            _capi.require_device(vis, "target joints2D_vis")
            if vis.dtype not in (torch.bool, torch.uint8):
                raise _capi.HpsError("joints2D_vis must be a bool (or uint8) tensor")
            vis = vis.contiguous()
            vis = vis.view(torch.uint8) if vis.dtype == torch.bool else vis
            if ps.dim() != 4 or ps.shape[0] != t2.shape[0] or tuple(ps.shape[2:]) != tuple(t2.shape[1:]) or tuple(vis.shape) != tuple(t2.shape[:2]):
                raise _capi.HpsError("joints2Dsamples must be (B, N, K, 2) and joints2D_vis (B, K) for joints2D (B, K, 2): got %s, %s, %s"
                                     % (tuple(ps.shape), tuple(vis.shape), tuple(t2.shape)))
            keep += [ps, vis]
            a.pred_joints2d_samples, a.vis, a.N = _capi.ptr(ps), _capi.ptr(vis, torch.uint8), ps.shape[1]
        if B is None:
            B = 1
        if status is not None:
            a.status, a.num_status = _capi.iptr(status, "status"), status.numel()

        if loss.dtype != torch.float32 or loss.numel() != 1:
            raise _capi.HpsError("loss must be one float32 on the device")
        loss = loss.detach()
        dev = loss.device
        if self._sums is None or self._sums.device != dev:
            self._sums = torch.zeros(2, NSLOT, device=dev, dtype=torch.float64)
        ws = self._ws.get(B)
        if ws is None or ws.device != dev:
            ws = self._ws[B] = torch.empty(_capi.query_workspace(_capi.WS_TRAIN_METRICS, B) // 8, device=dev, dtype=torch.float64)
        a.B, a.batch_size, a.mask, a.split, a.img_wh = B, int(batch_size), mask, SPLITS.index(split), float(self.img_wh)
        a.loss, a.workspace, a.sums = _capi.ptr(loss), _capi.ptr(ws, torch.float64), _capi.ptr(self._sums, torch.float64)
        _capi.call("hps_train_metrics_update", ctypes.byref(a), _capi.stream())
        # (a converted copy in ``keep`` is freed here: it was made on the current stream, whose order the allocator keeps)

    def update_per_epoch(self):
        """:198-236: one read-back of the device sums, then the epoch's per-sample values are appended to ``epochs_history`` (0 for
        a metric that is not tracked), printed, and the history is pickled as plain Python floats."""
        if self._sums is None:
            raise _capi.HpsError("update_per_epoch() without an update_per_batch() since the tracker was made")
        sums = self._sums.cpu().tolist()                                     # the epoch's one synchronisation
        L = self.loss_metric_sums
        for row, split in zip(sums, SPLITS):
            L[split + '_losses'] = row[SLOT_LOSS]
            L[split + '_num_samples'] = int(row[SLOT_SAMPLES])
            for i, name in enumerate(METRIC_NAMES):
                L[split + '_' + name] = row[SLOT_METRIC0 + i]
            L[split + '_num_visib_joints2Dsamples'] = row[SLOT_VISIBLE]
        bad = int(sums[0][SLOT_STATUS] + sums[1][SLOT_STATUS])
        if bad:
            raise _capi.HpsError("no body pixel left to determine the bounding box of %d image(s) of this epoch (the reference raises at "
                                 "utils/image_utils.py:304); their crop was the whole frame" % bad)
        H = self.epochs_history
        for split in SPLITS:
            H[split + '_losses'].append(L[split + '_losses'] / L[split + '_num_samples'])
        for metric_type in self.all_metrics_types:
            split, name = metric_type.split('_', 1)
            if name not in self.metrics_to_track:
                H[metric_type].append(0.)
            elif name == 'joints2Dsamples-L2E':
                visible = L[split + '_num_visib_joints2Dsamples']          # no visible joint in the epoch: the reference's 0 / 0, nan
                H[metric_type].append(L[metric_type] / visible if visible else float('nan'))
            else:
                per_sample = self._per_sample['PVE' if 'PVE' in name else 'MPJPE' if 'MPJPE' in name else 'joints2D']
                H[metric_type].append(L[metric_type] / (L[split + '_num_samples'] * per_sample))
        print('Finished epoch.')
        print('Train Loss: {:.5f}, Val Loss: {:.5f}'.format(H['train_losses'][-1], H['val_losses'][-1]))
        for name in self.metrics_to_track:
            print('Train {}: {:.5f}, Val {}: {:.5f}'.format(name, H['train_' + name][-1], name, H['val_' + name][-1]))
        if self.log_save_path is not None:
            with open(self.log_save_path, 'wb') as f_out:
                pickle.dump(H, f_out)

    def determine_save_model_weights_this_epoch(self, save_val_metrics, best_epoch_val_metrics):
        """:238-245: True unless a metric of ``save_val_metrics`` got worse than the best epoch's."""
        return all(self.epochs_history['val_' + m][-1] <= best_epoch_val_metrics[m] for m in save_val_metrics)
