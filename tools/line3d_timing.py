"""Per-call time of drfe_lines_is_good_batch next to the host entry drfe_lines_is_good looped over the same frames on one CPU
thread and on 16: 1, 8, 64 and 512 frames of 640 x 480 (synthetic room frames, their key lines from lsd_extract_batch, 40 a frame
at most, the frames repeated with seeds 1 .. F), k_as_f64 = 1.  The device call is timed with the depth images in host memory
(they are uploaded inside the call) and already on the device.  The clock is around the C entries alone; the device call returns
with the results in host memory.  Every shape is called once before it is timed and repeated until --seconds have been timed.
Device == host is checked for every frame.  Prints one JSON line per size and writes a table to --out
(profiles/line3d_batch.txt).  --trace F: only three device calls of F frames (depth on the device) after a warm-up one, for a
`rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, seconds, max_reps):
    fn()
    ts = []
    while (sum(ts) < seconds and len(ts) < max_reps) or len(ts) < 5:
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return [round(1e3 * float(f(ts)), 4) for f in (np.median, np.min, np.max)] + [len(ts)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--max-reps", type=int, default=100)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 8, 64, 512])
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line3d_batch.txt"))
    args = ap.parse_args()
    import torch
    from dr_slam_amd import lib, synth
    cam = synth.TUM3
    ctx = lib.Context(max_batch=1)          # fails without a GPU: there is no other way to measure the device
    L = lib.load()
    K9 = np.array([cam.fx, 0, cam.cx, 0, cam.fy, cam.cy, 0, 0, 1], np.float32)
    invfx, invfy = np.float32(1) / np.float32(cam.fx), np.float32(1) / np.float32(cam.fy)
    src = list(synth.sequence(2, args.distinct))
    ext = ctx.lsd_extract_batch(np.stack([g for g, _, _ in src]), max_lines=40)
    depth0 = np.stack([d.astype(np.float32) * (np.float32(1) / np.float32(cam.depth_factor)) for _, d, _ in src])
    lines0 = np.zeros((args.distinct, 40), lib.KEYLINE_DTYPE)
    for f, e in enumerate(ext):
        lines0[f, :len(e["lines"])] = e["lines"]
    counts0 = np.array([len(e["lines"]) for e in ext], np.int32)
    rows = []
    try:
        for F in ([args.trace] if args.trace else args.frames):
            pick = np.arange(F) % args.distinct
            lines, counts, depth = lines0[pick], counts0[pick], np.ascontiguousarray(depth0[pick])
            seeds = np.arange(1, F + 1, dtype=np.uint32)
            ddev = torch.from_numpy(depth).cuda()
            cam_args = (K9, cam.cx, cam.cy, invfx, invfy)
            fh, oh, rh, keep_h = lib.line3d_frames(lines, counts, depth, *cam_args, seeds=seeds)
            fd, od, rd, keep_d = lib.line3d_frames(lines, counts, ddev, *cam_args, seeds=seeds)

            def dev(fr=fh, out=oh):
                if L.drfe_lines_is_good_batch(ctx.h, C.byref(fr), C.byref(out), None) != 0:
                    raise RuntimeError("drfe_lines_is_good_batch failed")

            if args.trace:
                for _ in range(4):
                    dev(fd, od)
                continue
            want = (np.full((F, 40), -1, np.float32), np.zeros((F, 40, 6)), np.zeros((F, 40), np.int32), np.zeros(F, np.int32))
            kl, dl, l3, ni, ng = keep_h[0], want[0], want[1], want[2], want[3]

            def host_frames(lo, hi):
                for f in range(lo, hi):
                    good = C.c_int()
                    rc = L.drfe_lines_is_good(kl[f].ctypes.data, int(counts[f]), depth[f].ctypes.data, cam.w, cam.h, cam.w,
                                              K9.ctypes.data, 1, C.c_float(cam.cx), C.c_float(cam.cy), C.c_float(invfx),
                                              C.c_float(invfy), int(seeds[f]), dl[f].ctypes.data, l3[f].ctypes.data,
                                              ni[f].ctypes.data, C.byref(good))
                    if rc != 0:
                        raise RuntimeError("drfe_lines_is_good failed")
                    ng[f] = good.value

            pool = ThreadPoolExecutor(args.threads)
            cuts = np.linspace(0, F, min(args.threads, F) + 1).astype(int)

            def host_threads():
                list(pool.map(lambda k: host_frames(cuts[k], cuts[k + 1]), range(len(cuts) - 1)))

            t_dev = timed(dev, args.seconds, args.max_reps)
            t_ondev = timed(lambda: dev(fd, od), args.seconds, args.max_reps)
            t_host = timed(lambda: host_frames(0, F), args.seconds, args.max_reps)
            t_pool = timed(host_threads, args.seconds, args.max_reps)
            pool.shutdown()
            for got in (rh, rd):
                for a, b in zip(got, want):
                    assert a.tobytes() == b.tobytes(), F
            row = dict(frames=F, lines=int(counts.sum()), accepted=int(ng.sum()), device_host_depth_ms=t_dev, device_ms=t_ondev,
                       host_1_thread_ms=t_host, host_threads=args.threads, host_threads_ms=t_pool,
                       speedup_vs_1_thread=round(t_host[0] / t_ondev[0], 2), speedup_vs_threads=round(t_pool[0] / t_ondev[0], 2))
            print(json.dumps(row), flush=True)
            rows.append(row)
        stats = ctx.line3d_stats()
    finally:
        ctx.close()
    if args.trace:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("drfe_lines_is_good_batch against drfe_lines_is_good looped on the host; 640 x 480, k_as_f64 = 1; ms per call as\n"
                "median / min / max (calls timed); tools/line3d_timing.py\n\n")
        f.write("frames | lines | accepted | device, depth on the host | device, depth on the device | host, 1 thread | host, "
                f"{args.threads} threads | 1 thread / device | {args.threads} threads / device\n")
        cell = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f} ({t[3]})"  # noqa: E731
        for r in rows:
            f.write(f"{r['frames']} | {r['lines']} | {r['accepted']} | {cell(r['device_host_depth_ms'])} | {cell(r['device_ms'])} | "
                    f"{cell(r['host_1_thread_ms'])} | {cell(r['host_threads_ms'])} | {r['speedup_vs_1_thread']}x | "
                    f"{r['speedup_vs_threads']}x\n")
        f.write("\ncounters over the run: " + json.dumps(stats) + "\n")


if __name__ == "__main__":
    main()
