"""Seeded cases, restatements and accuracy rules of the training loss-and-metrics tracker's tests (tests/test_train_tracker_host.py,
tests/test_gpu_train_tracker.py): csrc/metrics.hip (hps_train_metrics_update) under train_loss_and_metrics_tracker.  Nothing here
touches a device; cases and references are computed once and shared (callers must not modify them).

A CASE is one batch: predicted and target vertices and reposed vertices (B, P, 3), joints (B, J, 3), normalised predicted 2-D joints
(B, K, 2) and their N samples (B, N, K, 2), target 2-D joints in pixels (B, K, 2), a visibility (B, K) and a loss, all float32 (vis
bool).  Predictions are noisy similarity transforms of their targets, far from them compared with every bound.

RESTATEMENT.  ``Restated(metrics, img_wh, dtype)`` is the reference's update_per_batch / update_per_epoch
(metrics/train_loss_and_metrics_tracker.py:113-236) with every array and every running sum in ``dtype``, the alignments by
eval_scenario.similarity_transform / scale_and_translation (the reference's utils/eval_utils.py as oracle/ref_cpu.py states it).  The
float64 one is the truth; the float32 one gives e32.  The loss sum is the reference's own in both: float(loss) * batch_size in Python
floats.  tests/golden/train_tracker_golden.json pins the restatement to the reference's class itself (make_train_tracker_golden.py).

RULES, this project's usual one.
  history values:  |value - r64| <= 4 * max(|r32 - r64|, 2**-23 * |r64|)
  point-set sums:  eval_scenario's bound_sum = sqrt(3) * P * 4 * max(e32 of the points, 2**-23 * scale), summed over the sets
  2-D sums:        4 * max(e32, 2**-23 * max(|coordinate|, img_wh)) per joint, times the number of joints in the sum; e32 the largest
                   float32-restatement error of one joint's distance
"""
import functools
import math

import numpy as np

import eval_scenario as E

EPS32 = E.EPS32
METRICS = ('PVE', 'PVE-SC', 'PVE-PA', 'PVE-T', 'PVE-T-SC', 'MPJPE', 'MPJPE-SC', 'MPJPE-PA', 'joints2D-L2E', 'joints2Dsamples-L2E')
SPLITS = ('train', 'val')
NSLOT = 14
SLOT_LOSS, SLOT_SAMPLES, SLOT_METRIC0, SLOT_VISIBLE, SLOT_STATUS = 0, 1, 2, 12, 13
# metric -> (family, mode): families 0 vertices, 1 reposed vertices, 2 joints
POINT_METRICS = {'PVE': (0, E.MODE_RAW), 'PVE-SC': (0, E.MODE_SC), 'PVE-PA': (0, E.MODE_PA), 'PVE-T': (1, E.MODE_RAW),
                 'PVE-T-SC': (1, E.MODE_SC), 'MPJPE': (2, E.MODE_RAW), 'MPJPE-SC': (2, E.MODE_SC), 'MPJPE-PA': (2, E.MODE_PA)}
FAMILY_KEYS = (('pred_verts', 'target_verts'), ('pred_reposed', 'target_reposed'), ('pred_joints3d', 'target_joints3d'))
VIS_MODES = ('some', 'per_image', 'one_image_none', 'none', 'all')
GOLDEN = dict(seeds=(11, 12, 13, 14), splits=('train', 'val', 'train', 'val'), B=2, P=6890, J=14, K=17, N=3, img_wh=256)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _noisy_similar(rs, t, noise):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    R = q * np.sign(np.linalg.det(q))
    return (0.7 + 0.6 * rs.rand()) * t.dot(R.T) + 0.2 * rs.randn(3) + noise * rs.randn(*t.shape)


@functools.lru_cache(maxsize=None)
def case(seed, B, P, J=14, K=17, N=3, img_wh=256, vis_mode='some'):
    """One batch (read-only arrays).  ``vis_mode``: 'some' (about a quarter invisible), 'per_image' (image b sees joints k with
    (k + b) % (b + 2) != 0), 'one_image_none' (image 0 sees nothing), 'none', 'all'."""
    rs = np.random.RandomState(77000 + seed)
    c = dict(seed=seed, B=B, P=P, J=J, K=K, N=N, img_wh=img_wh, vis_mode=vis_mode)
    for (pk, tk), n in zip(FAMILY_KEYS, (P, P, J)):
        target = np.stack([0.3 * rs.randn(n, 3) for _ in range(B)])
        c[tk], c[pk] = _f32(target), _f32(np.stack([_noisy_similar(rs, t, 0.05) for t in target]))
    c['target_joints2d'] = _f32(rs.rand(B, K, 2) * img_wh)
    mode_px = c['target_joints2d'] + rs.randn(B, K, 2) * 6.0
    samples_px = c['target_joints2d'][:, None] + rs.randn(B, N, K, 2) * 9.0
    c['pred_joints2d'] = _f32(mode_px / (img_wh / 2.0) - 1.0)
    c['pred_joints2d_samples'] = _f32(samples_px / (img_wh / 2.0) - 1.0)
    if vis_mode == 'some':
        vis = rs.rand(B, K) > 0.25
    elif vis_mode == 'per_image':
        vis = np.array([[(k + b) % (b + 2) != 0 for k in range(K)] for b in range(B)])
    elif vis_mode == 'one_image_none':
        vis = rs.rand(B, K) > 0.25
        vis[0] = False
    else:
        vis = np.full((B, K), vis_mode == 'all')
    c['vis'] = np.ascontiguousarray(vis, dtype=bool)
    c['loss'] = np.float32(3.0 + rs.rand())
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def pointset_case_of(c, family):
    """The family's point sets as an eval_scenario case (group 1), for its reference and bounds."""
    pk, tk = FAMILY_KEYS[family]
    return dict(name=None, pred=c[pk], target=c[tk], group=1, S=c[pk].shape[0], P=c[pk].shape[1])


def aligned(c, family, mode, dtype):
    """(B, n, 3) ``dtype``: the family's predictions after the mode's alignment."""
    return E.transformed(pointset_case_of(c, family), mode, dtype)


def j2d_errors(c, dtype, samples):
    """Per-joint distances in pixels, ``dtype``: (B, K), or (B, N, K) for the samples -- (x + 1) * (img_wh / 2) - target, :176-193."""
    pred = c['pred_joints2d_samples'] if samples else c['pred_joints2d']
    target = c['target_joints2d'][:, None] if samples else c['target_joints2d']
    px = (pred.astype(dtype) + dtype(1)) * dtype(c['img_wh'] / 2.0)
    out = np.linalg.norm(px - target.astype(dtype), axis=-1)
    assert out.dtype == dtype
    return out


class Restated:
    """The reference's tracker arithmetic in ``dtype`` (module docstring).  ``sums[split][name]``: the running sums under the
    reference's names without the split prefix ('losses', 'num_samples', the metrics, 'num_visib_joints2Dsamples')."""

    def __init__(self, metrics, img_wh, dtype):
        self.metrics, self.img_wh, self.dtype = list(metrics), img_wh, dtype
        self.history = {'%s_%s' % (s, m): [] for m in ('losses',) + METRICS for s in SPLITS}
        self.start_epoch()

    def start_epoch(self):
        self.sums = {s: dict({m: self.dtype(0) for m in METRICS}, losses=0.0, num_samples=0, num_visib_joints2Dsamples=self.dtype(0))
                     for s in SPLITS}
        self.sizes = {}

    def update(self, split, c, batch_size):
        dt, sums = self.dtype, self.sums[split]
        sums['losses'] += float(c['loss']) * batch_size
        sums['num_samples'] += batch_size
        for m, (family, mode) in POINT_METRICS.items():
            if m in self.metrics:
                target = c[FAMILY_KEYS[family][1]].astype(dt)
                err = np.linalg.norm(aligned(c, family, mode, dt) - target, axis=-1)
                assert err.dtype == dt
                sums[m] = dt(sums[m] + np.sum(err))
                self.sizes[m.split('-')[0]] = target.shape[1]
        if 'joints2D-L2E' in self.metrics:
            sums['joints2D-L2E'] = dt(sums['joints2D-L2E'] + np.sum(j2d_errors(c, dt, False)))
            self.sizes['joints2D'] = c['K']
        if 'joints2Dsamples-L2E' in self.metrics:
            keep = np.broadcast_to(c['vis'][:, None, :], (c['B'], c['N'], c['K']))
            sums['joints2Dsamples-L2E'] = dt(sums['joints2Dsamples-L2E'] + np.sum(j2d_errors(c, dt, True)[keep]))
            sums['num_visib_joints2Dsamples'] = dt(sums['num_visib_joints2Dsamples'] + int(keep.sum()))

    def end_epoch(self):
        for s in SPLITS:
            sums = self.sums[s]
            self.history[s + '_losses'].append(sums['losses'] / sums['num_samples'])
            for m in METRICS:
                if m not in self.metrics:
                    value = 0.0
                elif m == 'joints2Dsamples-L2E':
                    with np.errstate(invalid='ignore', divide='ignore'):
                        value = sums[m] / sums['num_visib_joints2Dsamples']
                else:
                    value = sums[m] / (sums['num_samples'] * self.sizes['joints2D' if m == 'joints2D-L2E' else m.split('-')[0]])
                self.history['%s_%s' % (s, m)].append(float(value))
        return self.history


def run_restated(updates, metrics, img_wh, dtype, batch_size=None):
    """History after one epoch of ``updates`` = [(split, case), ...]."""
    r = Restated(metrics, img_wh, dtype)
    for split, c in updates:
        r.update(split, c, c['B'] if batch_size is None else batch_size)
    return r.end_epoch(), r


def history_bound(r64, r32):
    """The rule for one history value."""
    return 4.0 * max(abs(r32 - r64), EPS32 * abs(r64))


def golden_updates():
    g = GOLDEN
    return [(split, case(seed, g['B'], g['P'], g['J'], g['K'], g['N'], g['img_wh'], 'some')) for seed, split in zip(g['seeds'], g['splits'])]


# ---- the device's per-set values and sums ----
@functools.lru_cache(maxsize=None)
def _pointset_bound(seed, B, P, J, K, N, img_wh, vis_mode, family, mode):
    """(float64 truth of the family's per-set error sums (B,), bound on their total) by eval_scenario's rule, summed over the sets."""
    c = case(seed, B, P, J, K, N, img_wh, vis_mode)
    pc = pointset_case_of(c, family)
    q64, q32 = E.transformed(pc, mode, np.float64), E.transformed(pc, mode, np.float32)
    e32 = float(np.abs(q32.astype(np.float64) - q64).max())
    scale = float(max(np.abs(q64).max(), np.abs(pc['pred']).max()))
    bound_set = math.sqrt(3.0) * pc['P'] * 4.0 * max(e32, EPS32 * scale)
    return E.error_sums(q64, E.targets(pc)), bound_set * pc['S']


def pointset_truth(c, family, mode):
    return _pointset_bound(c['seed'], c['B'], c['P'], c['J'], c['K'], c['N'], c['img_wh'], c['vis_mode'], family, mode)


def j2d_truth(c, samples):
    """(float64 sum, bound on it, number of joints in it) of joints2D-L2E (all joints) or joints2Dsamples-L2E (visible joints of every
    sample)."""
    e64, e32 = j2d_errors(c, np.float64, samples), j2d_errors(c, np.float32, samples)
    keep = np.broadcast_to(c['vis'][:, None, :], e64.shape) if samples else np.ones(e64.shape, dtype=bool)
    pred = c['pred_joints2d_samples'] if samples else c['pred_joints2d']
    coord = max(float(np.abs((pred.astype(np.float64) + 1) * c['img_wh'] / 2.0).max()), float(np.abs(c['target_joints2d']).max()), float(c['img_wh']))
    per_joint = 4.0 * max(float(np.abs(e32.astype(np.float64) - e64).max()), EPS32 * coord)
    n = int(keep.sum())
    return float(e64[keep].sum()), per_joint * n, n


def replica_sums(running, split, per_set, j2d, loss, batch_size, mask, status=None):
    """The finishing workgroup on the host: ``running`` (2, NSLOT) float64 -> a new array.  ``per_set`` (3, B, 3) and ``j2d`` (B, 3)
    are the device's workspace values; each tracked column is added up in set order in float64 from 0.0, then running + value."""
    out = np.array(running, dtype=np.float64, copy=True)
    row = out[SPLITS.index(split)]

    def column(values):
        total = np.float64(0.0)
        for v in values:
            total = total + np.float64(v)
        return total

    row[SLOT_LOSS] += np.float64(np.float32(loss)) * np.float64(batch_size)
    row[SLOT_SAMPLES] += np.float64(batch_size)
    for i, m in enumerate(METRICS):
        if not (mask >> i) & 1:
            continue
        if m in POINT_METRICS:
            family, mode = POINT_METRICS[m]
            row[SLOT_METRIC0 + i] += column(per_set[family, :, mode])
        else:
            row[SLOT_METRIC0 + i] += column(j2d[:, i - 8])
    if (mask >> 9) & 1:
        row[SLOT_VISIBLE] += column(j2d[:, 2])
    if status is not None:
        row[SLOT_STATUS] += column([1.0 if s else 0.0 for s in status])
    return out
