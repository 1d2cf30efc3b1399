"""Per-batch preparation of a training batch, B = 72 and img_wh = 256, on one MI355X: OnTheFlySMPLTrainDataset.prepare_batch (uint8
items -> one pinned staging buffer -> one copy -> hps_texture_gather + hps_resize_bilinear_u8) against the same batch composed the
reference's way from the same decoded arrays (data/on_the_fly_smpl_train_dataset.py:79-94 per item: NumPy ``/ 255.`` in float64 ->
``.float()``, then default_collate and ``.to(device)``).

Image decoding is common to both routes and reported on its own (PIL, per background).  The reference resizes each background with
cv2.resize on the host; OpenCV is not a dependency here, so that one call is stood in for by PIL's bilinear resize of the same image
-- its cost is reported separately too, and the host route is given both with and without it.

Two warm-up rounds of each route, then ROUNDS rounds with the routes alternated; a round is timed by the host clock around the calls
and a final synchronise; median and quartiles per batch.

    python tools/data_layer_time.py
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from torch.utils.data import default_collate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hierarchicalprobabilistic3dhuman_amd.on_the_fly_smpl_train_dataset import OnTheFlySMPLTrainDataset  # noqa: E402

B, WH = 72, 256
N_GREY, N_NONGREY, N_BACKGROUNDS = 2, 10, 24
BG_H, BG_W = 256, 341                                    # LSUN images as distributed: the shorter side is 256
ROUNDS, WARMUP = 9, 2


def write_files(root):
    from PIL import Image
    rs = np.random.RandomState(0)
    os.makedirs(os.path.join(root, "backgrounds"))
    np.savez(os.path.join(root, "poses.npz"), fnames=np.array(["amass_%d" % i for i in range(B)]), poses=(rs.randn(B, 72) * 0.2).astype(np.float32))
    np.savez(os.path.join(root, "textures.npz"), grey=rs.randint(0, 256, (N_GREY, 1200, 800, 3)).astype(np.uint8),
             nongrey=rs.randint(0, 256, (N_NONGREY, 1200, 800, 3)).astype(np.uint8))
    for i in range(N_BACKGROUNDS):
        base = rs.rand(BG_H // 8, BG_W // 8 + 1, 3)      # 8 x 8 blocks plus per-pixel noise
        img = (np.kron(base, np.ones((8, 8, 1)))[:BG_H, :BG_W] * 200 + rs.randint(0, 56, (BG_H, BG_W, 3))).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "backgrounds", "bg_%03d.jpg" % i), quality=90)
    return dict(poses_path=os.path.join(root, "poses.npz"), textures_path=os.path.join(root, "textures.npz"),
                backgrounds_dir_path=os.path.join(root, "backgrounds"))


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": statistics.median(ms), "q1_ms": q[0], "q3_ms": q[2]}


def main():
    from PIL import Image
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with tempfile.TemporaryDirectory() as root:
        ds = OnTheFlySMPLTrainDataset(img_wh=WH, **write_files(root))
        torch.manual_seed(0)
        t0 = time.perf_counter()
        items = [ds[i] for i in range(B)]
        decode_ms = (time.perf_counter() - t0) * 1e3     # B x (three draws + one JPEG decode)
    backgrounds = [it["background"].numpy() for it in items]
    t0 = time.perf_counter()
    resized = [np.asarray(Image.fromarray(bg).resize((WH, WH), Image.BILINEAR)) for bg in backgrounds]
    host_resize_ms = (time.perf_counter() - t0) * 1e3

    def reference_route(with_resize):
        samples = []
        for it, bg, small in zip(items, backgrounds, resized):
            g, idx = it["texture_choice"]
            texture = (ds.grey_textures if g else ds.nongrey_textures)[idx]
            if with_resize:
                small = np.asarray(Image.fromarray(bg).resize((WH, WH), Image.BILINEAR))
            samples.append({"pose": it["pose"], "texture": torch.from_numpy(texture / 255.).float(),
                            "background": torch.from_numpy(small.transpose(2, 0, 1) / 255.).float()})
        batch = default_collate(samples)
        return {k: v.to(dev) for k, v in batch.items()}

    routes = (("device", lambda: ds.prepare_batch(items)), ("host", lambda: reference_route(False)),
              ("host_with_resize", lambda: reference_route(True)))
    a, b = routes[0][1](), routes[1][1]()
    torch.cuda.synchronize()
    same = {k: bool(torch.equal(a[k], b[k])) for k in ("pose", "texture")}
    bg_diff = float((a["background"] - b["background"]).abs().max() * 255)
    print("routes agree: %s; backgrounds differ by at most %.2f levels (PIL's resize is not cv2's)" % (same, bg_diff), flush=True)
    for _ in range(WARMUP):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in routes}
    for _ in range(ROUNDS):
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {"B": B, "img_wh": WH, "rounds": ROUNDS, "decode_ms_per_batch": decode_ms, "host_resize_stand_in_ms_per_batch": host_resize_ms,
           "texture_and_pose_equal": same, "background_max_level_diff_vs_stand_in": bg_diff}
    for name, _ in routes:
        out[name] = stats(ms[name])
    out["uint8_bytes_copied_per_batch"] = int(sum(bg.nbytes for bg in backgrounds) + B * 72 * 4)
    out["float32_bytes_of_the_batch"] = int(sum(v.numel() * 4 for v in a.values()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
