"""Per-frame time of the device Manhattan-frame tracker (drfe_manhattan_track_batch, 3 calls per frame) at 640x480 for several
batch shapes, next to the host entry (drfe_manhattan_track_host, one CPU thread) on the same frames, and the download of
the records the host path would need.  Prints one JSON line per configuration (and writes them to the file given with --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from dr_slam_amd import lib, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cam = synth.TUM3
    frames = list(synth.sequence(2, a.frames, cam=cam, kind="room_boxes"))
    Rcw = np.linalg.inv(frames[0][2])[:3, :3].astype(np.float32)
    K4 = (cam.fx, cam.fy, cam.cx, cam.cy)
    inv = np.float32(1.0) / np.float32(cam.depth_factor)
    lines = []
    stream = torch.cuda.Stream()          # a stream of its own: stream 0 would send the calls to the context's stream
    c = lib.Context()
    try:
        for nseq, seq_len in ((1, 64), (8, 16), (64, 1), (64, 8), (256, 4)):
            nf = nseq * seq_len
            depth = torch.from_numpy(np.stack([frames[i % len(frames)][1] for i in range(nf)]).view(np.int16)).cuda()
            torch.cuda.synchronize()
            c.surface_normals_batch_ptr(depth.data_ptr(), cam.w * cam.h, cam.w, cam.w, cam.h, K4, inv, 9.0, nf, stream.cuda_stream)
            R0 = np.stack([Rcw] * nseq)
            ms = []
            for r in range(a.reps + 1):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c.manhattan_track_batch(R0, nseq, seq_len, None, None, 3, stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                if r:
                    ms.append(e0.elapsed_time(e1))
            # the host path: download every frame's records, then the host entry chained the same way (one thread)
            t0 = time.perf_counter()
            recs = [c.surface_normals_download(f) for f in range(nf)]
            t1 = time.perf_counter()
            for s in range(nseq):
                R = Rcw
                for t in range(seq_len):
                    R = lib.manhattan_track_host(R, recs[s * seq_len + t])[0]
            t2 = time.perf_counter()
            rec = dict(w=cam.w, h=cam.h, nseq=nseq, seq_len=seq_len, frames=nf, device_batch_ms_median=float(np.median(ms)),
                       device_ms_per_frame=float(np.median(ms)) / nf, device_ms_min=float(min(ms)),
                       download_ms_per_frame=1e3 * (t1 - t0) / nf, host_ms_per_frame=1e3 * (t2 - t1) / nf)
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
