"""Creates a context, runs the frame-batch entries on 64 frames (lines, AHC and CAPE planes) and one call of every other device
path that owns buffers (surface normals + Manhattan tracking, plane maps: upload, match, update, the ORB matchers, BoW), closes
it - five times - and prints the device memory in use after each round (a leak of an arena shows as a step)."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dr_slam_amd import lib, synth, vocabulary
from dr_slam_amd.pipeline import FrontEnd
cam = synth.ICL
frames = list(synth.sequence(3, 8, cam=cam, kind="living_room"))
gray = np.stack([frames[i % 8][0] for i in range(64)]); depth = np.stack([frames[i % 8][1] for i in range(64)])
K4 = np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float32); inv = float(np.float32(1.0) / np.float32(cam.depth_factor))
depth_m = depth.astype(np.float32) * np.float32(inv)
Twc = np.stack([f[2] for f in frames[:2]]).astype(np.float64)
Tcw = np.linalg.inv(Twc).astype(np.float32); Twc = Twc.astype(np.float32)
rng = np.random.default_rng(0)
coefs = np.array([[0, 0, 1, -2.0], [1, 0, 0, -0.5], [0, 1, 0, -0.3], [0.6, 0.8, 0, -2.0]], np.float32)
clouds = [rng.random((300, 3)).astype(np.float32) for _ in coefs]
plane_map = dict(coefs=coefs, bad=np.zeros(len(coefs), np.uint8), clouds=clouds, points=np.vstack(clouds)[::5].copy())
voc = vocabulary.make_synthetic(6, 4, seed=3)
torch.cuda.init()
for r in range(5):
    ctx = lib.Context(max_batch=2)
    ctx.lsd_extract_batch(gray, n_threads=4); ctx.planes_ahc_post_batch(depth, K4, inv, 9.0, 0.10, n_threads=4); ctx.planes_cape_batch(depth_m, K4, 20, n_threads=2)
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.from_numpy(gray[:2]).cuda(); d = torch.from_numpy(depth[:2].view(np.int16)).cuda()
    ctx.surface_normals_batch_ptr(d.data_ptr(), cam.w * cam.h, cam.w, cam.w, cam.h, K4, inv, 9.0, 2, stream)
    ctx.manhattan_track_batch(np.repeat(np.eye(3, dtype=np.float32)[None], 2, 0), 2, 1, stream=stream)
    ctx.plane_map_upload([plane_map])
    ctx.plane_match_batch([0], Tcw[:1], [coefs], flag_points=True, stream=stream)
    ctx.plane_map_update_batch([0], Tcw[:1], [[c[::2].copy() for c in clouds]], map_idx=None, stream=stream)
    fe = FrontEnd(cam, max_batch=2, ctx=ctx)
    fe.process(g, d, Tcw, Twc, stream=stream)
    n_last, n_cur = len(fe.keypoints(0)[0]), len(fe.keypoints(1)[0])
    mp = np.zeros(n_last, lib.MAPPOINT_DTYPE)
    mp["valid"], mp["obs_positive"], mp["desc"] = 1, 1, fe.keypoints(0)[1]
    mp["world"] = (np.c_[rng.random((n_last, 2)) - 0.5, np.full(n_last, 2.0)] @ Twc[0][:3, :3].T + Twc[0][:3, 3]).astype(np.float32)
    ctx.search_by_projection_last(1, 0, Tcw[1], Tcw[0], fe.cam, mp, n_cur)
    voc.upload(ctx)
    ctx.bow_transform_batch(2, 2, stream)
    torch.cuda.synchronize()
    free_in, total = torch.cuda.mem_get_info()
    ctx.close()
    free_out, _ = torch.cuda.mem_get_info()
    print("round %d: in use with the context %.2f GB, after close %.2f GB" % (r, (total - free_in) / 2**30, (total - free_out) / 2**30), flush=True)
