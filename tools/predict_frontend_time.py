"""The predict front end, image to network input, on one MI355X: predict_frontend.DevicePredictFrontEnd on a batch against the
per-image route (predict_hrnet + image_utils.batch_crop_pytorch_affine + proxy_representation, the body of
predict_poseMF_shapeGaussian_net._reference_front_end) looped over the same images, both with the same device HRNet-W48 (seeded
weights) at 384 x 288 and PROXY_REP_SIZE 256, on 720 x 960 uint8 photographs that are resident on the device, no person detector.

B = 1, 4 and 16; three warm-up rounds of each route, then 20 rounds with the routes alternated; a round is timed by the host clock
around the calls and a final synchronise (the per-image route waits on the host by itself), reported per image as median and quartiles.
Kernel launches per image of both routes come from one profiled round each, after the timing.

    python tools/predict_frontend_time.py
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import hrnet_scenario as S  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd import configs  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.image_utils import batch_crop_pytorch_affine  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import PoseHighResolutionNet  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.predict_frontend import DevicePredictFrontEnd  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.predict_hrnet import predict_hrnet  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.predict_poseMF_shapeGaussian_net import proxy_representation  # noqa: E402

H, W = 960, 720
ROUNDS, WARMUP = 20, 3


def per_image_route(chw_u8, hrnet, hrnet_cfg, edge, cfg, dev):
    """predict_poseMF_shapeGaussian_net._reference_front_end's body from the uploaded (3,H,W) uint8 image on."""
    D = cfg.DATA.PROXY_REP_SIZE
    image = chw_u8.float() / 255.0
    hr = predict_hrnet(hrnet_model=hrnet, hrnet_config=hrnet_cfg, object_detect_model=None, image=image,
                       object_detect_threshold=cfg.DATA.BBOX_THRESHOLD, bbox_scale_factor=cfg.DATA.BBOX_SCALE_FACTOR)
    crop_h, crop_w = hr["cropped_image"].shape[1:]
    centre = torch.tensor([[crop_h, crop_w]], dtype=torch.float32, device=dev) * 0.5
    height = torch.tensor([crop_h], dtype=torch.float32, device=dev)
    cropped = batch_crop_pytorch_affine(input_wh=(hrnet_cfg.MODEL.IMAGE_SIZE[0], hrnet_cfg.MODEL.IMAGE_SIZE[1]), output_wh=(D, D),
                                        num_to_crop=1, device=dev, joints2D=hr["joints2D"][None], rgb=hr["cropped_image"][None],
                                        bbox_centres=centre, bbox_heights=height, bbox_widths=height.clone(), orig_scale_factor=1.0)
    visib = hr["joints2Dconfs"] > 0.75
    visib[[0, 1, 2, 3, 4, 5, 6, 11, 12]] = True
    return proxy_representation(cropped["rgb"], cropped["joints2D"], visib[None], edge, cfg)


def count_kernels(fn):
    """Device kernels of one call, from torch's profiler; None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = 0
        for ev in prof.events():
            if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
                n += 1
        return n
    except Exception as e:                                     # a tool's optional figure must not lose the timings
        print("kernel count not measured: %s" % e, flush=True)
        return None


def main():
    dev = torch.device("cuda:0")
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "hrnet_w48_keys.json")))
    sd = S.seeded_state_dict({k: (tuple(s), d) for k, s, d in keys}, S.W48_SEED)
    hrnet_cfg = S.config("W48")
    hrnet = PoseHighResolutionNet(hrnet_cfg).eval()
    hrnet.load_state_dict(sd, strict=True)
    hrnet = hrnet.to(dev)
    cfg = configs.get_cfg_defaults()
    edge = CannyEdgeDetector(non_max_suppression=cfg.DATA.EDGE_NMS, gaussian_filter_std=cfg.DATA.EDGE_GAUSSIAN_STD,
                             gaussian_filter_size=cfg.DATA.EDGE_GAUSSIAN_SIZE, threshold=cfg.DATA.EDGE_THRESHOLD).to(dev)
    front = DevicePredictFrontEnd(cfg, hrnet, hrnet_cfg, edge, None, 0.75, dev)
    rs = np.random.RandomState(0)
    out = {}
    with torch.no_grad():
        for B in (1, 4, 16):
            photos = []
            for _ in range(B):
                # 8 x 8 blocks plus per-pixel noise
                base = rs.rand(H // 8, W // 8, 3)
                photos.append((np.kron(base, np.ones((8, 8, 1))) * 200 + rs.randint(0, 56, (H, W, 3))).astype(np.uint8))
            hwc = [torch.from_numpy(p).to(dev) for p in photos]
            chw = [torch.from_numpy(np.ascontiguousarray(p.transpose(2, 0, 1))).to(dev) for p in photos]
            routes = (("batched", lambda: front(hwc)["proxy_rep"]),
                      ("per_image", lambda: [per_image_route(c, hrnet, hrnet_cfg, edge, cfg, dev) for c in chw]))
            a, b = routes[0][1](), torch.cat(routes[1][1]())
            # channel 0 holds the thinned edges' gradient MAGNITUDES (zero elsewhere): presence and value are compared separately
            flips = float(((a[:, 0] != 0) != (b[:, 0] != 0)).float().mean())
            print("B=%d  routes agree: heat-map channels max|diff| = %.3e; edge map: %.2f %% of the pixels are edges, presence differs on "
                  "%.4f %%, max|magnitude diff| = %.3e" % (B, float((a[:, 1:] - b[:, 1:]).abs().max()), 100 * float((a[:, 0] != 0).float().mean()),
                                                          100 * flips, float((a[:, 0] - b[:, 0]).abs().max())), flush=True)
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
                    ms[name].append((time.perf_counter() - t0) * 1e3 / B)
            res = {}
            for name, _ in routes:
                q = statistics.quantiles(ms[name], n=4)
                res[name + "_ms_per_image"], res[name + "_q"] = statistics.median(ms[name]), (q[0], q[2])
            out["B%d" % B] = res
            print("B=%d" % B, res, flush=True)
        for B in (1, 16):
            hwc = [torch.from_numpy(np.zeros((H, W, 3), dtype=np.uint8)).to(dev) for _ in range(B)]
            chw = [t.permute(2, 0, 1).contiguous() for t in hwc]
            nb = count_kernels(lambda: front(hwc))
            npi = count_kernels(lambda: [per_image_route(c, hrnet, hrnet_cfg, edge, cfg, dev) for c in chw])
            out["B%d" % B]["launches_per_image"] = {"batched": None if nb is None else nb / B, "per_image": None if npi is None else npi / B,
                                                    "hrnet_forward": hrnet.launches_per_forward(B, 384, 288, dev)}
            print("B=%d launches per image" % B, out["B%d" % B]["launches_per_image"], flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
