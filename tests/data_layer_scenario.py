"""Cases and NumPy restatements for the device data layer (csrc/data_layer.hip, data_layer.py): cv2.resize(INTER_LINEAR) and
cv2.warpAffine on uint8 in integer arithmetic, a float64 ideal bilinear for both, the crop's matrix and the heat-map formula of the
reference.  The warp's positions are tests/vis_scenario.warp_positions -- one reading of cv2.warpAffine for the whole suite.

Two kinds of image: NOISE (uniform random bytes; every bit of the integer arithmetic matters -- for the bit-for-bit comparisons) and
SMOOTH (neighbouring pixels differ by a few levels -- for the comparison with the float64 ideal, see ``SMOOTH_STEP``).
"""
import numpy as np

from vis_scenario import warp_positions

K = 17
ALWAYS_VISIBLE = (0, 1, 2, 3, 4, 5, 6, 11, 12)

# resize: (H, W) sources and (out_h, out_w) targets.  1 x 1 and 1 x 9 (every tap clamped), 7 x 5 (up, odd), 32 x 32 (exactly 2x at 16:
# OpenCV's INTER_AREA switch, same levels), 37 x 53 (down, odd, rows not 4-byte aligned), 300 x 200 (non-square, down and up)
RESIZE_SOURCES = ((1, 1), (1, 9), (7, 5), (32, 32), (37, 53), (300, 200))
RESIZE_TARGETS = (16, 256)

# A SMOOTH image changes by at most SMOOTH_STEP levels between neighbouring pixels (either axis).  The warp places a sample on a 1/32
# pixel lattice (5 bits; positions are rounded, so off by at most 1/64 per axis, plus 2^-10 from the 10-bit row / column terms): the
# value moves by at most 2 * SMOOTH_STEP * (1/64 + 2^-10) < 0.26 levels, the final rounding adds 1/2: within one level.  The resize's
# 11-bit coefficients (sum exactly 2048) move a row sum by at most SMOOTH_STEP / 4096 levels per axis; its two truncations lose less
# than 1/4 level each and the rounding offset is 1/2: within one level as well.
SMOOTH_STEP = 8


def noise_image(seed, H, W, channels=3):
    rs = np.random.RandomState(seed)
    shape = (H, W, channels) if channels else (H, W)
    return rs.randint(0, 256, shape).astype(np.uint8)


def smooth_image(seed, H, W):
    """(H, W, 3) uint8: a sum of low-frequency waves, neighbouring pixels at most SMOOTH_STEP apart (asserted)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        fy, fx, ph = rs.uniform(0.01, 0.045, 2).tolist() + [rs.uniform(0, 6.28)]
        img[:, :, c] = 127.5 + 60.0 * np.sin(fy * y + ph) + 60.0 * np.cos(fx * x - ph)
    out = np.rint(img).astype(np.uint8)
    for axis in (0, 1):
        if out.shape[axis] > 1:
            assert np.abs(np.diff(out.astype(np.int64), axis=axis)).max() <= SMOOTH_STEP
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cv2.resize(INTER_LINEAR), uint8
# ---------------------------------------------------------------------------------------------------------------------------------
def _resize_axis(dst, src, column):
    """Per output index: (i0, i1, c0, c1) int64 -- taps and 11-bit coefficients."""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (float(src) / float(dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    if column:                                    # the position becomes the edge pixel with fraction 0
        low = s < 0
        f, s = np.where(low, np.float32(0), f), np.where(low, 0, s)
        high = s >= src - 1
        f, s = np.where(high, np.float32(0), f), np.where(high, src - 1, s)
        i0, i1 = s, np.minimum(s + 1, src - 1)
    else:                                         # the two rows are clamped, the fraction is kept
        i0, i1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    f = f.astype(np.float32)
    c0 = np.clip(np.rint((np.float32(1) - f) * np.float32(2048)), -32768, 32767).astype(np.int64)
    c1 = np.clip(np.rint(f * np.float32(2048)), -32768, 32767).astype(np.int64)
    return i0, i1, c0, c1


def resize_levels(src, out_w, out_h):
    """(H, W, 3) uint8 -> (out_h, out_w, 3) uint8: cv2.resize(src, (out_w, out_h), interpolation=cv2.INTER_LINEAR) as we read it."""
    S = np.asarray(src).astype(np.int64)
    x0, x1, a0, a1 = _resize_axis(out_w, S.shape[1], True)
    y0, y1, b0, b1 = _resize_axis(out_h, S.shape[0], False)
    h = S[:, x0] * a0[None, :, None] + S[:, x1] * a1[None, :, None]                       # (H, out_w, 3)
    h0, h1 = h[y0], h[y1]
    level = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return (level & 255).astype(np.uint8)


def ideal_resize(src, out_w, out_h):
    """Float64 bilinear with half-pixel centres and a replicated edge: (out_h, out_w, 3) float64 levels."""
    S = np.asarray(src).astype(np.float64)
    H, W = S.shape[:2]

    def axis(dst, n):
        p = (np.arange(dst) + 0.5) * (n / float(dst)) - 0.5
        p = np.clip(p, 0.0, n - 1.0)
        i0 = np.minimum(np.floor(p).astype(np.int64), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), p - i0
    x0, x1, fx = axis(out_w, W)
    y0, y1, fy = axis(out_h, H)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = S[y0][:, x0] * (1 - fx) + S[y0][:, x1] * fx
    bot = S[y1][:, x0] * (1 - fx) + S[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


# ---------------------------------------------------------------------------------------------------------------------------------
# the crop: utils/image_utils.py:145-229 with bbox_whs, no augmentation
# ---------------------------------------------------------------------------------------------------------------------------------
def crop_matrix(centre, side, scale_factor, wh):
    """image_utils.py:102, :145-194 as NumPy evaluates them on float64 labels: the (2,3) float32 matrix."""
    output_wh = np.array((wh, wh), dtype=np.float32)
    bbox_centre = np.asarray(centre, dtype=np.float64)
    bbox_height = bbox_width = np.float64(side)
    bbox_height = bbox_height * scale_factor
    bbox_width = bbox_width * scale_factor
    output_centre = output_wh * 0.5
    affine_trans = np.zeros((2, 3), dtype=np.float32)
    affine_trans[0, 0] = output_wh[0] / bbox_width
    affine_trans[1, 1] = output_wh[1] / bbox_height
    affine_trans[:, 2] = output_centre - (output_wh / np.array([bbox_width, bbox_height])) * bbox_centre[::-1]
    return affine_trans


def crop_joints(M, joints2D):
    """image_utils.py:212-214: (K,2) float64."""
    homo = np.concatenate([joints2D, np.ones((joints2D.shape[0], 1))], axis=-1)
    return np.einsum('ij,kj->ki', M, homo)


def _tap(src, y, x):
    h, w = src.shape[:2]
    inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    v = src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
    return np.where(inside[..., None] if v.ndim == 3 else inside, v, 0)


def crop_levels(src, M, wh):
    """(H, W, 3) uint8 -> (wh, wh, 3) uint8: cv2.warpAffine(src, M, (wh, wh), flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, 0).
    The 15-bit weight table holds exactly 32 (32 - fy)(32 - fx), ...: no adjustment, (sum + 2^14) >> 15 = (sum / 32 + 512) >> 10."""
    p = warp_positions(M, wh, wh)
    S = np.asarray(src).astype(np.int64)
    fx, fy = p["fx"][..., None], p["fy"][..., None]
    sy, sx = p["sy"], p["sx"]
    total = (_tap(S, sy, sx) * ((32 - fy) * (32 - fx)) + _tap(S, sy, sx + 1) * ((32 - fy) * fx) +
             _tap(S, sy + 1, sx) * (fy * (32 - fx)) + _tap(S, sy + 1, sx + 1) * (fy * fx))
    return ((total + 512) >> 10).astype(np.uint8)


def crop_nearest(seg, M, wh):
    """(H, W) uint8 -> (wh, wh) uint8, INTER_NEAREST, constant border 0."""
    p = warp_positions(M, wh, wh)
    return _tap(np.asarray(seg).astype(np.int64), p["ny"], p["nx"]).astype(np.uint8)


def ideal_crop(src, M, wh):
    """Float64 bilinear at the exact inverse positions, zero outside: ((wh, wh, 3) levels, mask of samples whose four taps all lie
    inside the image or all outside -- at the image's edge the zero border is a step of up to 255 levels, where a 1/64 pixel moves the
    value by up to 4)."""
    S = np.asarray(src).astype(np.float64)
    H, W = S.shape[:2]
    m = np.asarray(M, dtype=np.float32).astype(np.float64)
    j, i = np.meshgrid(np.arange(wh, dtype=np.float64), np.arange(wh, dtype=np.float64))
    x, y = (j - m[0, 2]) / m[0, 0], (i - m[1, 2]) / m[1, 1]
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    v = (_tap(S, y0, x0) * (1 - fy) * (1 - fx) + _tap(S, y0, x0 + 1) * (1 - fy) * fx + _tap(S, y0 + 1, x0) * fy * (1 - fx) +
         _tap(S, y0 + 1, x0 + 1) * fy * fx)
    # a margin of one pixel: the fixed-point position may fall into the neighbouring cell
    inside = (x >= 1) & (x <= W - 2) & (y >= 1) & (y <= H - 2)
    outside = (x < -2) | (x > W + 1) | (y < -2) | (y > H + 1)
    return v, inside | outside


def crop_boxes(H, W):
    """(centre (vertical, horizontal), side): inside, partly outside on each side, larger than the image, centred on a corner."""
    s = float(min(H, W))
    return {"inside": ((H / 2.0 + 0.3, W / 2.0 - 1.7), 0.55 * s), "off_top": ((0.1 * H, W / 2.0), 0.7 * s),
            "off_bottom": ((0.93 * H, W / 2.0 + 0.25), 0.7 * s), "off_left": ((H / 2.0, 0.08 * W), 0.7 * s),
            "off_right": ((H / 2.0 - 0.5, 0.95 * W), 0.7 * s), "larger": ((H / 2.0, W / 2.0), 1.9 * max(H, W)),
            "corner": ((0.0, 0.0), 0.8 * s), "far_corner": ((float(H), float(W)), 0.5 * s)}


CROP_IMAGES = ((1, 1), (41, 67), (90, 60))      # 1 x 1 and non-square, both orientations


def crop_keypoints(seed, H, W):
    """(17, 3) float64: x, y, confidence -- inside, outside, and confidences on both sides of a threshold of 0.5 and at it."""
    rs = np.random.RandomState(seed)
    kp = np.empty((K, 3))
    kp[:, 0], kp[:, 1] = rs.uniform(-0.3 * W, 1.3 * W, K), rs.uniform(-0.3 * H, 1.3 * H, K)
    kp[:, 2] = rs.uniform(0, 1, K)
    kp[7, 2], kp[8, 2], kp[9, 2], kp[0, 2] = 0.5, 0.49, 0.51, 0.1          # 0.5 is NOT > 0.5; joint 0 is always visible
    return kp


# ---------------------------------------------------------------------------------------------------------------------------------
# heat maps: utils/label_conversions.py:89-102 and the visibility rule of the two evaluation datasets
# ---------------------------------------------------------------------------------------------------------------------------------
def heatmaps(positions, img_wh, std, dtype=np.float32, confidence=None, threshold=None):
    """positions (K, 2) integers -> (K, img_wh, img_wh); dtype float32 is the reference's own arithmetic, float64 the ideal."""
    xx, yy = np.meshgrid(np.arange(img_wh), np.arange(img_wh))
    xx, yy = xx[None].astype(dtype), yy[None].astype(dtype)
    j = np.asarray(positions).astype(np.int16).astype(dtype)
    u, v = j[:, 0, None, None], j[:, 1, None, None]
    std = dtype(std)
    heat = np.exp(-(((xx - u) / std) ** 2) / 2 - (((yy - v) / std) ** 2) / 2)
    if threshold is not None:
        flag = np.asarray(confidence) > threshold
        flag[list(ALWAYS_VISIBLE)] = True
        heat = heat * flag[:, None, None]
    return heat


# integer positions from float64 key points: truncation toward zero (SSP-3D) and round-half-to-even (3DPW)
POSITION_PROBES = np.array([[-0.7, 0.7], [-1.0, -1.5], [-2.5, 2.5], [0.5, 1.5], [3.5, -0.5], [-0.2, 255.9], [12.49, 12.51],
                            [-3.999, 7.0]], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# synthetic dataset directories (built in a temporary directory at test time) and the draw-order fixture's parameters
# ---------------------------------------------------------------------------------------------------------------------------------
DRAW_SEEDS, DRAW_BATCHES = (0, 1, 7), (1, 4, 9)
DRAW_N_GREY, DRAW_N_NONGREY, DRAW_N_BACKGROUNDS, DRAW_GREY_PROB = 2, 3, 5, 0.4
POSE_FNAMES = ("h36m_0", "amass_a", "up3d_1", "3dpw_2", "amass_b", "h36m_3", "other_4")


def write_train_files(root, seed=0, marker_textures=False, background_sizes=((24, 30), (16, 16), (33, 20), (8, 40), (19, 19))):
    """poses.npz, textures.npz (grey: DRAW_N_GREY, nongrey: DRAW_N_NONGREY, 1200 x 800 x 3 uint8) and backgrounds/bg_<i>.jpg under
    ``root``.  marker_textures: texture i of the grey bank is filled with i, of the non-grey bank with 100 + i."""
    import os
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "backgrounds"), exist_ok=True)
    np.savez(os.path.join(root, "poses.npz"), fnames=np.array(POSE_FNAMES), poses=rs.randn(len(POSE_FNAMES), 72).astype(np.float32) * 0.2)
    if marker_textures:
        grey = np.stack([np.full((1200, 800, 3), i, np.uint8) for i in range(DRAW_N_GREY)])
        nongrey = np.stack([np.full((1200, 800, 3), 100 + i, np.uint8) for i in range(DRAW_N_NONGREY)])
    else:
        grey = rs.randint(0, 256, (DRAW_N_GREY, 1200, 800, 3)).astype(np.uint8)
        nongrey = rs.randint(0, 256, (DRAW_N_NONGREY, 1200, 800, 3)).astype(np.uint8)
    np.savez(os.path.join(root, "textures.npz"), grey=grey, nongrey=nongrey)
    for i, (h, w) in enumerate(background_sizes[:DRAW_N_BACKGROUNDS]):
        Image.fromarray(smooth_image(100 + i, h, w)).save(os.path.join(root, "backgrounds", "bg_%d.jpg" % i), quality=95)
    open(os.path.join(root, "backgrounds", "notes.txt"), "w").write("not a background\n")
    return dict(poses_path=os.path.join(root, "poses.npz"), textures_path=os.path.join(root, "textures.npz"),
                backgrounds_dir_path=os.path.join(root, "backgrounds"))


def write_ssp3d_files(root, n=5, seed=0, sizes=((60, 44), (48, 48), (41, 67), (52, 70), (64, 40))):
    """images/, silhouettes/ (PNG: decoded exactly) and labels.npz for ``n`` frames of different sizes under ``root``."""
    import os
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "silhouettes"), exist_ok=True)
    fnames, kps, centres, whs = [], [], [], []
    for i in range(n):
        H, W = sizes[i % len(sizes)]
        name = "frame_%02d.png" % i
        Image.fromarray(noise_image(seed * 100 + i, H, W)).save(os.path.join(root, "images", name))
        yy, xx = np.mgrid[0:H, 0:W]
        blob = ((yy - H / 2.0) ** 2 / (0.4 * H) ** 2 + (xx - W / 2.1) ** 2 / (0.25 * W) ** 2) <= 1.0
        Image.fromarray((blob * 255).astype(np.uint8)).save(os.path.join(root, "silhouettes", name))
        fnames.append(name)
        kps.append(crop_keypoints(seed * 100 + i, H, W))
        centres.append((H / 2.0 + rs.uniform(-3, 3), W / 2.0 + rs.uniform(-3, 3)))
        whs.append(0.8 * max(H, W) + rs.uniform(0, 4))
    np.savez(os.path.join(root, "labels.npz"), fnames=np.array(fnames), shapes=rs.randn(n, 10).astype(np.float32),
             poses=(rs.randn(n, 72) * 0.2).astype(np.float32), joints2D=np.stack(kps), bbox_centres=np.array(centres),
             bbox_whs=np.array(whs), genders=np.array(["m", "f"] * n)[:n])
    return root


def write_pw3d_files(root, n=4, seed=0, sides=(40, 64, 33, 256), non_square=None):
    """cropped_frames/ (PNG), 3dpw_test.npz and hrnet_results_centred.npy under ``root``; frame ``non_square`` is made (S, S + 3)."""
    import os
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "cropped_frames"), exist_ok=True)
    names, kps = [], []
    for i in range(n):
        S = sides[i % len(sides)]
        name = "crop_%02d.png" % i
        Image.fromarray(noise_image(seed * 100 + 50 + i, S, S + (3 if non_square == i else 0))).save(os.path.join(root, "cropped_frames", name))
        names.append(name)
        kp = crop_keypoints(seed * 100 + 50 + i, S, S)
        kp[:POSITION_PROBES.shape[0], :2] = POSITION_PROBES * (S / 16.0)       # ties at wh = 16: x * 16 / S lands on the probes
        kps.append(kp)
    np.savez(os.path.join(root, "3dpw_test.npz"), imgname=np.array(names), pose=(rs.randn(n, 72) * 0.2).astype(np.float32),
             shape=rs.randn(n, 10).astype(np.float32), gender=np.array(["f", "m"] * n)[:n])
    np.save(os.path.join(root, "hrnet_results_centred.npy"), np.stack(kps))
    return root
