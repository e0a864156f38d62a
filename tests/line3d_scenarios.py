"""The hand-built scene of the isLineGood tests (test_line3d_cpu.py, test_gpu_line3d.py): a 160 x 120 depth image with
fx = fy = 200, cx = 80, cy = 60 - a slanted wall up to x = 100 and a step behind it - with sensor noise, 15 % outliers, the
1/5000 m quantisation of a depth PNG and a hole, and twelve key lines that reach every branch of the 3-D lifting: the integer
sample rule with its border clamp, 9 and 10 samples, a sub-pixel line, samples outside the image and in the hole, 51 samples,
and one line twice so that the rand() chain shows.  Without the noise every line would exit at its first RANSAC iteration."""
import numpy as np

W, H = 160, 120
FX = FY = 200.0
CX, CY = 80.0, 60.0
K9 = np.array([FX, 0, CX, 0, FY, CY, 0, 0, 1], np.float32)
INVFX = np.float32(1) / np.float32(FX)
INVFY = np.float32(1) / np.float32(FY)

# (sx, sy, ex, ey)
SEGMENTS = (
    (10.3, 20.7, 70.9, 25.2),     # an ordinary line
    (60.2, 50.3, 140.7, 52.1),    # across the step
    (0, 7, 12, 7),                # all-integer samples at the border; two samples land on one pixel through the clamp
    (20.1, 30.2, 28.6, 30.4),     # 9 samples: skipped, no draws
    (20.1, 35.2, 29.6, 35.4),     # exactly 10 samples
    (50.1, 40.1, 50.5, 40.3),     # a sub-pixel line
    (-20.5, 80.3, 40.2, 85.1),    # partly outside the image
    (10.2, 100.3, 80.8, 101.9),   # through the hole
    (5.5, 110.2, 150.3, 112.8),   # more than 50 px: 51 samples
    (30.5, 10.5, 30.5, 60.5),     # vertical
    (12, 9, 0, 9),                # the border case reversed
    (10.3, 20.7, 70.9, 25.2),     # line 0 again, at the end
)


def depth_image():
    """float32 [H, W] in metres"""
    x = np.arange(W, dtype=np.float64)
    z = np.where(x < 100, 2 + 0.002 * x, 4.0)[None, :].repeat(H, 0)
    rng = np.random.default_rng(3)
    z = z + rng.normal(0, 0.02, (H, W))
    out = rng.random((H, W)) < 0.15
    z = z + np.where(out, rng.uniform(0.2, 1.0, (H, W)), 0.0)
    z = np.round(z * 5000) / 5000
    z[95:111, 30:36] = 0
    return z.astype(np.float32)


def key_lines(dtype, segments=SEGMENTS, count=None):
    """the segments as `count` key lines (default: each once; more: repeated in order); only the end points are read"""
    count = len(segments) if count is None else count
    kl = np.zeros(count, dtype)
    for i in range(count):
        sx, sy, ex, ey = segments[i % len(segments)]
        kl[i]["start_point_x"], kl[i]["start_point_y"], kl[i]["end_point_x"], kl[i]["end_point_y"] = sx, sy, ex, ey
        kl[i]["pt_x"], kl[i]["pt_y"] = (sx + ex) / 2, (sy + ey) / 2
        kl[i]["class_id"] = i
    return kl
