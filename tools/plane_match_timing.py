"""Per-frame time of device plane association (drfe_plane_match_batch with flag_points: SearchMapByCoefficients, then
FlagMatchedPlanePoints) against one resident map of up to 200 planes, 20 k-point clouds and 100 k map points, at 1, 64 and 256
frames per call, next to the host entries (drfe_plane_match_host + drfe_plane_flag_points_host, one CPU thread) on the same
frames, and the per-frame download.  Prints one JSON line per configuration (and writes them to the file given with --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def observe(map_coefs, rng, P):
    """a random pose and P camera-frame planes near planes of the map"""
    a = rng.normal(0, 0.3, 3)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Tcw = np.eye(4)
    Tcw[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    Tcw[:3, 3] = rng.normal(0, 1, 3)
    Tcw = Tcw.astype(np.float32)
    w = map_coefs[rng.integers(0, len(map_coefs), P)].astype(np.float64)
    w[:, :3] += rng.normal(0, 0.02, (P, 3))
    w[:, 3] += rng.normal(0, 0.08, P)
    return Tcw, (np.linalg.inv(Tcw.astype(np.float64)).T @ w.T).T.astype(np.float32)


def main():
    import torch
    import plane_match_numpy as PN
    from dr_slam_amd import lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-planes", type=int, default=200)
    ap.add_argument("--cloud", type=int, default=20000, help="largest cloud (uniform in [0, cloud))")
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--planes", type=int, default=10, help="planes per frame")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=16, help="frames timed on the host per configuration")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    _, _, mc, bad, clouds, pts = PN.random_scene(11, a.map_planes, a.planes, a.cloud, a.points)
    rng = np.random.default_rng(5)
    lines = []
    stream = torch.cuda.Stream()          # a stream of its own: stream 0 would send the calls to the context's stream
    c = lib.Context()
    try:
        c.plane_map_upload([dict(coefs=mc, bad=bad, clouds=clouds, points=pts)])
        for nf in (1, 64, 256):
            obs = [observe(mc, rng, a.planes) for _ in range(nf)]
            T = np.stack([o[0] for o in obs])
            cf = [o[1] for o in obs]
            ms = []
            for r in range(a.reps + 1):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c.plane_match_batch([0] * nf, T, cf, flag_points=True, stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                if r:
                    ms.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            for f in range(nf):
                c.plane_match_download(f)
            flags = c.plane_flags_download(0)
            t1 = time.perf_counter()
            nh = min(nf, a.host_frames)
            for f in range(nh):
                mi = lib.plane_match_host(obs[f][0], obs[f][1], mc, bad, clouds)[0]
                lib.plane_flag_points_host(obs[f][0], obs[f][1], mi, pts)
            t2 = time.perf_counter()
            rec = dict(map_planes=len(mc), cloud_points=int(sum(len(x) for x in clouds)), map_points=len(pts), planes_per_frame=a.planes,
                       frames=nf, device_batch_ms_median=float(np.median(ms)), device_ms_per_frame=float(np.median(ms)) / nf,
                       device_ms_min=float(min(ms)), download_ms_per_frame=1e3 * (t1 - t0) / nf,
                       host_ms_per_frame=1e3 * (t2 - t1) / nh, host_frames=nh, flagged_points=int(flags.sum()))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    finally:
        c.close()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
