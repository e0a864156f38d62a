"""-m gpu tests of the device chain drfe_surface_normals(_batch) -> drfe_manhattan_track_batch on the hand-built scenarios of
tests/normals_manhattan_scenarios.py (DESIGN.md sections 9 and 11).  tests/test_normals_manhattan_edges_cpu.py proves on the
host that every scenario reaches the branch or seam it names; here the same scenarios go through the device and everything is
compared bit for bit, without a tolerance:

A. Surface normals.  The float single-frame entry with its taps against the oracle (cloud, normals, records: NaN in the same
   places, identical float bits elsewhere, identical frame positions) and its `dist` tap against the plain numpy chamfer
   transform of the scenarios module; the batch entry on device-resident uint16 depth, tightly packed and with padded row and
   frame strides (padding 65535), against the oracle and against each other.  The oracle defines non-finite depth, so the
   non-finite frame is held to it like every other (float entry only: it is not uint16-representable).
B. Manhattan tracking on the records those frames leave on the device: R, info, record bits and line bits of every frame equal
   the host entry fed the downloaded records and chained frame to frame, equal the numpy restatement on every frame, and give
   the answers the scenario states by hand.

All tests share one context, so every call also runs on buffers an earlier, differently sized call left behind."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manhattan_numpy as MN  # noqa: E402
import normals_manhattan_scenarios as S  # noqa: E402
from test_normals_manhattan_edges_cpu import (MANHATTAN, NORMALS, bits, check_expect, check_records, oracle_normals,  # noqa: E402
                                              same_floats)

pytestmark = pytest.mark.gpu
U16 = [sc["name"] for sc in S.normals_scenarios() if sc["d16"] is not None]


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context()
    yield c
    c.close()


def normals_batch(c, buf, frame_stride, row_stride, cam, maxd, nframes):
    """drfe_surface_normals_batch on a host buffer put on the device -> the records of every frame"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(buf, np.uint16).reshape(-1).view(np.int16)).cuda()
    assert t.numel() >= (nframes - 1) * frame_stride + (cam.h - 1) * row_stride + cam.w
    c.surface_normals_batch_ptr(t.data_ptr(), frame_stride, row_stride, cam.w, cam.h, cam.K4, S.INV, maxd, nframes,
                                torch.cuda.current_stream().cuda_stream)
    return [c.surface_normals_download(f) for f in range(nframes)]


@pytest.mark.parametrize("name", NORMALS)
def test_float_entry_equals_oracle_and_numpy_chamfer(ctx, oracle_mod, name):
    sc = S.normals_scenarios()[NORMALS.index(name)]
    cam = sc["cam"]
    cloud, nrm, recs = oracle_normals(oracle_mod, sc["depth_m"], cam.K4, sc["maxd"])
    rec, dcloud, dnrm, ddist = ctx.surface_normals(sc["depth_m"], cam.K4, sc["maxd"], taps=True)
    assert same_floats(dcloud, cloud)
    assert same_floats(dnrm, nrm)
    check_records(rec, recs)
    assert np.array_equal(bits(ddist), bits(S.scenario_dist(sc)))


@pytest.mark.parametrize("name", U16)
def test_batch_entry_tight_and_padded_equals_oracle(ctx, oracle_mod, name):
    """two frames side by side (the scenario and its point reflection), tightly packed and with row_stride = w + 5,
    frame_stride = row_stride * h + 7"""
    sc = S.normals_scenarios()[NORMALS.index(name)]
    cam = sc["cam"]
    frames = np.stack([sc["d16"], np.ascontiguousarray(sc["d16"][::-1, ::-1])])
    want = [oracle_normals(oracle_mod, S.to_metres(d), cam.K4, sc["maxd"])[2] for d in frames]
    tight = normals_batch(ctx, frames, cam.w * cam.h, cam.w, cam, sc["maxd"], 2)
    buf, fs, rs = S.padded(frames)
    assert rs == cam.w + 5 and fs == rs * cam.h + 7 and (buf.reshape(2, fs)[:, rs * cam.h:] == 65535).all()
    pad = normals_batch(ctx, buf, fs, rs, cam, sc["maxd"], 2)
    for f in range(2):
        check_records(tight[f], want[f])
        check_records(pad[f], want[f])
        assert pad[f].tobytes() == tight[f].tobytes()


@pytest.mark.parametrize("name", MANHATTAN)
def test_device_tracking_equals_host_and_numpy(ctx, oracle_mod, name):
    import torch
    from dr_slam_amd import lib
    sc = S.manhattan_scenarios()[MANHATTAN.index(name)]
    cam = sc["cam"]
    nf = len(sc["depth"])
    recs = normals_batch(ctx, sc["depth"], cam.w * cam.h, cam.w, cam, S.MAXD, nf)
    for f in range(nf):
        check_records(recs[f], oracle_normals(oracle_mod, S.to_metres(sc["depth"][f]), cam.K4, S.MAXD)[2])
    stream = torch.cuda.current_stream().cuda_stream
    for ci, call in enumerate(sc["calls"]):
        lines = len(call["dirs"]) > 0
        ctx.manhattan_track_batch(call["R0"], call["nseq"], call["seq_len"], call["dirs"] if lines else None,
                                  call["loff"] if lines else None, call["n_calls"], stream)
        for s in range(call["nseq"]):
            R = call["R0"][s]
            for t in range(call["seq_len"]):
                f = s * call["seq_len"] + t
                who = (name, ci, f)
                d = call["dirs"][call["loff"][f]:call["loff"][f + 1]]
                Rd, infod, rbd, lbd = ctx.manhattan_download(f, len(recs[f]))
                Rh, infoh, rbh, lbh = lib.manhattan_track_host(R, recs[f], d, call["n_calls"])
                assert np.array_equal(bits(Rd), bits(Rh)), (who, Rd, Rh)
                assert infod.tobytes() == infoh.tobytes(), (who, infod, infoh)
                assert np.array_equal(rbd, rbh) and np.array_equal(lbd, lbh), who
                Rn, infos, rbn, lbn, _ = MN.track(R, recs[f]["normal"], d, call["n_calls"])
                MN.assert_equal_to_product(Rn, infos, rbn, lbn, Rd, infod, rbd, lbd)
                check_expect(call["expect"].get(f, {}), R, Rd, infod, rbd, lbd, who)
                R = Rd
