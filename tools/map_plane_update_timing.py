"""Per-call and per-frame time of device map-plane upkeep (drfe_plane_map_update_batch: the per-frame form of
MapPlane::UpdateCoefficientsAndPoints for every matched frame plane) on resident maps, next to the host entry
(drfe_map_plane_update_host, one CPU thread) on the same updates.  Configurations: 1 map x 1 frame, 64 and 256 maps x 1 frame
per call (one frame of every map), and the section-12 map of 200 planes with clouds up to 20 k points x 1 frame.  Each frame
updates --planes distinct planes of its map with its own plane clouds (the planes' points seen from the frame's pose, noisy,
so the clouds stay near their size), and the steps chain: step k updates the clouds step k - 1 left.  The device call returns
once the clouds are updated, so wall time is its cost.  Prints one JSON line per configuration (and writes them to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frame_of(rng, clouds, planes, frac=0.5):
    """a random pose Tcw and, for `planes` distinct map planes, a noisy camera-frame sample of their clouds"""
    import map_plane_numpy as MN
    Tcw = MN.random_pose(rng, 0.3)
    T = Tcw.astype(np.float64)
    idx = rng.choice(len(clouds), min(planes, len(clouds)), replace=False).astype(np.int32)
    fc = []
    for j in idx:
        w = clouds[j][rng.random(len(clouds[j])) < frac].astype(np.float64)
        w = w + rng.normal(0, 0.01, w.shape)
        fc.append(((T[:3, :3] @ w.T).T + T[:3, 3]).astype(np.float32))
    return Tcw, fc, idx


def main():
    import torch
    import plane_match_numpy as PN
    from dr_slam_amd import lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=10, help="updated planes per frame")
    ap.add_argument("--steps", type=int, default=4, help="timed calls per configuration (after one warm-up call)")
    ap.add_argument("--host-frames", type=int, default=16, help="frames timed on the host per configuration")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    configs = [("small", 1, 24, 3000), ("small", 64, 24, 3000), ("small", 256, 24, 3000), ("section12", 1, 200, 20000)]
    lines = []
    stream = torch.cuda.Stream()
    for name, nmaps, nplanes, cloud in configs:
        rng = np.random.default_rng(7)
        maps = []
        for s in range(nmaps):
            _, _, mc, bad, clouds, pts = PN.random_scene(1000 + s, nplanes, a.planes, cloud, 1000, special=False)
            maps.append(dict(coefs=mc, bad=bad, clouds=clouds, points=pts))
        host = [[c.copy() for c in m["clouds"]] for m in maps]
        c = lib.Context()
        try:
            c.plane_map_upload(maps)
            ms, hms, hn, npts = [], 0.0, 0, 0
            for step in range(a.steps + 1):
                fr = [frame_of(rng, host[s], a.planes) for s in range(nmaps)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c.plane_map_update_batch(list(range(nmaps)), np.stack([f[0] for f in fr]), [f[1] for f in fr],
                                         map_idx=[f[2] for f in fr], stream=stream.cuda_stream)
                t1 = time.perf_counter()
                if step:
                    ms.append(1e3 * (t1 - t0))
                npts += sum(len(x) for f in fr for x in f[1])
                # the host entry on the same updates (every map keeps its host clouds in step with the device)
                for s, (Tcw, fc, idx) in enumerate(fr):
                    t2 = time.perf_counter()
                    for q, j in enumerate(idx):
                        host[s][j] = lib.map_plane_update_host(Tcw, fc[q], host[s][j])
                    if step and hn < a.host_frames:
                        hms += 1e3 * (time.perf_counter() - t2)
                        hn += 1
            same = all(np.array_equal(c.plane_map_cloud_download(s, j).view(np.uint32), host[s][j].view(np.uint32))
                       for s in range(0, nmaps, max(1, nmaps // 8)) for j in range(nplanes))
            st = c.plane_map_update_stats()
        finally:
            c.close()
        rec = dict(config=name, maps=nmaps, map_planes=nplanes, largest_cloud=cloud, planes_per_frame=a.planes, frames_per_call=nmaps,
                   frame_points_per_call=npts // (a.steps + 1), device_ms_per_call_median=float(np.median(ms)), device_ms_min=float(min(ms)),
                   device_ms_per_frame=float(np.median(ms)) / nmaps, host_ms_per_frame=hms / max(hn, 1), host_frames=hn,
                   device_equals_host=bool(same), stats=st)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
