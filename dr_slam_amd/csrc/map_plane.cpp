/* map_plane.cpp — MapPlane::UpdateCoefficientsAndPoints (reference src/MapPlane.cc:298-371) behind the C-ABI of include/drfe.h:
 * the two host entries (no context) and the device entries on the resident maps of drfe_plane_map_upload (plane_match.cpp),
 * with the plane edits and the cloud download.  Both sides evaluate map_plane_core.h and the same pcl::VoxelGrid
 * (planes_post.cpp / voxel_kernels.hip); DESIGN.md section 13. */
#include "plane_map_internal.h"
#include "map_plane_core.h"

#include <cstring>

namespace {

const float kLeaf = 0.05f;          /* voxel.setLeafSize(0.05, 0.05, 0.05) */

bool offsets_ok(const int32_t* off, int n)
{
    if (off[0] < 0) return false;
    for (int i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    return true;
}

/* pcl::VoxelGrid(0.05) of xyz floats on the host (drfe_plane_voxel_grid); the result never holds more points than the input */
int voxel_host(const float* xyz, size_t n, std::vector<float>& out)
{
    static const float none[3] = {0.f, 0.f, 0.f};
    out.resize(std::max<size_t>(3 * n, 3));
    int m = 0;
    const int rc = drfe_plane_voxel_grid(n ? xyz : none, (int)n, kLeaf, out.data(), (int)n, &m);
    out.resize(3 * (size_t)std::max(m, 0));
    return rc;
}

int finish_host(const std::vector<float>& in, float* out_xyz, int cap, int* n_out)
{
    std::vector<float> v;
    int rc = voxel_host(in.data(), in.size() / 3, v);
    if (rc) return rc;
    *n_out = (int)(v.size() / 3);
    if (*n_out > cap) return DRFE_ERR_CAPACITY;
    if (*n_out > 0 && !out_xyz) return DRFE_ERR_INVALID;
    if (*n_out > 0) std::memcpy(out_xyz, v.data(), v.size() * 4);
    return DRFE_OK;
}

typedef MpJob Job;

/* new slots for every plane whose cloud may outgrow its slot (need[j] > cap[j]): a fresh arena, every cloud moved in */
int repack(drfe_ctx* c, PmBuffers* b, const std::vector<int64_t>& need, hipStream_t s)
{
    const size_t P = b->cntH.size();
    std::vector<int32_t> cap(P), beg(P);
    int64_t total = 0;
    int maxN = 0;
    std::vector<int4> mv;
    for (size_t j = 0; j < P; j++) {
        /* room for growth everywhere, so that a sequence repacks rarely: a plane that needs more gets half as much again,
         * every other plane twice its cloud */
        int64_t k = std::max<int64_t>(b->capH[j], 2 * (int64_t)b->cntH[j] + 256);
        if (need[j] > k) k = need[j] + need[j] / 2 + 256;
        if (k > INT32_MAX) { c->err = "plane_map: a cloud outgrows 2^31 points"; return DRFE_ERR_CAPACITY; }
        cap[j] = (int32_t)k;
        beg[j] = (int32_t)std::min<int64_t>(total, INT32_MAX);
        total += k;
        if (b->cntH[j] > 0) mv.push_back(make_int4(b->begH[j], beg[j], b->cntH[j], 0));
        maxN = std::max(maxN, b->cntH[j]);
    }
    if (total > INT32_MAX) { c->err = "plane_map: the clouds outgrow 2^31 points"; return DRFE_ERR_CAPACITY; }
    DevBuf<float> arena;
    HIPCHK(c, drfe_pm_reserve(arena, (size_t)total * 3));
    HIPCHK(c, drfe_pm_reserve(b->upMove, mv.size()));
    hipError_t e = hipSuccess;
    if (!mv.empty()) e = hipMemcpyAsync(b->upMove, mv.data(), mv.size() * sizeof(int4), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = drfe_launch_map_plane_move(b->upMove, (int)mv.size(), maxN, b->cloud, arena, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        c->err = std::string("plane_map repack: ") + hipGetErrorString(e);
        return DRFE_ERR_HIP;
    }
    b->cloud = std::move(arena);
    b->begH.swap(beg);
    b->capH.swap(cap);
    b->upStats[3]++;
    return drfe_pm_push_planes(c, b);
}

/* Runs the jobs in rounds: round r takes the r-th job of every plane, in call order.  Per round one staging copy, the gather,
 * the voxel grid and the commit, then the round's counts come back (4 bytes per job); a job the voxel grid handed back (grid
 * overflow, heap-sort branch, a loop bound) is redone on the host from its gathered input before the next round reads it. */
int run_jobs(drfe_ctx* c, PmBuffers* b, const std::vector<Job>& jobs, const std::vector<MpSeg>& segs, const float* poses, int nposes,
             const float* src, size_t nsrc, hipStream_t s)
{
    if (jobs.empty()) return DRFE_OK;
    std::vector<std::vector<int>> rounds;
    {
        std::vector<int> rank(b->cntH.size(), 0);
        for (int k = 0; k < (int)jobs.size(); k++) {
            const int r = rank[jobs[k].plane]++;
            if ((int)rounds.size() <= r) rounds.resize(r + 1);
            rounds[r].push_back(k);
        }
    }
    int rc;
    HIPCHK(c, drfe_pm_reserve(b->upSrc, nsrc * 3));
    HIPCHK(c, drfe_pm_reserve(b->upPose, (size_t)nposes * 16));
    if (nsrc) HIPCHK(c, hipMemcpyAsync(b->upSrc, src, nsrc * 12, hipMemcpyHostToDevice, s));
    if (nposes) HIPCHK(c, hipMemcpyAsync(b->upPose, poses, (size_t)nposes * 64, hipMemcpyHostToDevice, s));
    std::vector<float> hin, hout;
    for (const std::vector<int>& R : rounds) {
        const int nj = (int)R.size();
        std::vector<int64_t> n(nj);
        std::vector<int64_t> need(b->cntH.size(), 0);
        bool grow = false;
        int64_t total = 0;
        for (int i = 0; i < nj; i++) {
            const Job& J = jobs[R[i]];
            int64_t k = J.resident ? b->cntH[J.plane] : 0;
            for (int g = J.seg0; g < J.seg1; g++) k += segs[g].n;
            n[i] = k;
            total += k;
            need[J.plane] = k;
            grow |= k > b->capH[J.plane];
        }
        if (total > INT32_MAX) { c->err = "plane_map: a round's input outgrows 2^31 points"; return DRFE_ERR_CAPACITY; }
        if (grow && (rc = repack(c, b, need, s))) return rc;
        /* the round's records: segments, voxel jobs (offset, points), commits */
        std::vector<MpSeg> rs;
        std::vector<int2> vj(nj);
        std::vector<MpCommit> cm(nj);
        int32_t at = 0;
        int maxSeg = 0, maxJob = 0;
        for (int i = 0; i < nj; i++) {
            const Job& J = jobs[R[i]];
            vj[i] = make_int2(at, (int)n[i]);
            cm[i] = MpCommit{J.plane, at, b->begH[J.plane], b->capH[J.plane]};
            for (int g = J.seg0; g < J.seg1; g++) {
                MpSeg q = segs[g];
                q.dst = at;
                at += q.n;
                maxSeg = std::max(maxSeg, q.n);
                if (q.n) rs.push_back(q);
            }
            if (J.resident && b->cntH[J.plane] > 0) {
                MpSeg q{MP_SEG_RESIDENT, 0, b->begH[J.plane], b->cntH[J.plane], at, {0, 0, 0}};
                at += q.n;
                maxSeg = std::max(maxSeg, q.n);
                rs.push_back(q);
            }
            maxJob = std::max(maxJob, (int)n[i]);
        }
        StageLayout<16> lay;
        const auto sS = lay.add<MpSeg>(rs.size());
        const auto sJ = lay.add<int2>((size_t)nj);
        const auto sC = lay.add<MpCommit>((size_t)nj);
        const auto sK = lay.add<int>((size_t)nj);       /* the counts come back here: host block only, the copy up ends at sK.off */
        const size_t N = (size_t)total;
        HIPCHK(c, drfe_pm_reserve(b->upRec, sK.off));
        HIPCHK(c, drfe_pm_reserve(b->upHost, lay.bytes()));
        HIPCHK(c, drfe_pm_reserve(b->upIn, N * 3));
        HIPCHK(c, drfe_pm_reserve(b->upOut, N * 3));
        HIPCHK(c, drfe_pm_reserve(b->upRecs, N));
        HIPCHK(c, drfe_pm_reserve(b->upTmp, N));
        HIPCHK(c, drfe_pm_reserve(b->upPosL, N));
        HIPCHK(c, drfe_pm_reserve(b->upPosR, N));
        HIPCHK(c, drfe_pm_reserve(b->upList, (size_t)nj + 2));
        HIPCHK(c, drfe_pm_reserve(b->upCounts, (size_t)nj));
        char* h = b->upHost;
        sS.put(h, rs.data());
        sJ.put(h, vj.data());
        sC.put(h, cm.data());
        const char* d = b->upRec;
        HIPCHK(c, hipMemcpyAsync(b->upRec, h, sK.off, hipMemcpyHostToDevice, s));
        hipError_t e = drfe_launch_map_plane_gather(sS.at(d), (int)rs.size(), maxSeg, b->upPose, b->upSrc, b->cloud, b->upIn, s);
        if (e == hipSuccess)
            e = drfe_launch_voxel_grid(b->upIn, sJ.at(d), nj, b->upList, b->upRecs, b->upTmp, b->upPosL, b->upPosR,
                                       b->upOut, b->upCounts, kLeaf, s);
        if (e == hipSuccess)
            e = drfe_launch_map_plane_commit(sC.at(d), nj, maxJob, b->upCounts, b->upOut, b->cloud, b->cloudEnd, s);
        if (e != hipSuccess) { c->err = std::string("plane_map update: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
        int* counts = sK.at(h);
        HIPCHK(c, hipMemcpyAsync(counts, b->upCounts, (size_t)nj * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (int i = 0; i < nj; i++) {
            const int j = cm[i].plane;
            if (counts[i] >= 0 && counts[i] <= cm[i].cap) {
                b->cntH[j] = counts[i];
                b->upStats[0]++;
                continue;
            }
            hin.resize(3 * (size_t)n[i]);
            if (n[i]) HIPCHK(c, hipMemcpy(hin.data(), b->upIn + 3 * (size_t)vj[i].x, (size_t)n[i] * 12, hipMemcpyDeviceToHost));
            if ((rc = voxel_host(hin.data(), (size_t)n[i], hout))) { c->err = "plane_map update: host voxel grid failed"; return rc; }
            const int m = (int)(hout.size() / 3);
            if (m > cm[i].cap) { c->err = "plane_map update: voxel output exceeds its slot"; return DRFE_ERR_CAPACITY; }
            if (m) HIPCHK(c, hipMemcpy(b->cloud + 3 * (size_t)cm[i].dstBeg, hout.data(), (size_t)m * 12, hipMemcpyHostToDevice));
            const int32_t end = cm[i].dstBeg + m;
            HIPCHK(c, hipMemcpy(b->cloudEnd + j, &end, 4, hipMemcpyHostToDevice));
            b->cntH[j] = m;
            b->upStats[1]++;
        }
        b->upStats[2]++;
    }
    drfe_pm_chunks(b);                  /* the device's per-plane arrays are current: the commits and redos wrote the ends */
    return DRFE_OK;
}

PmBuffers* maps_of(drfe_ctx* c, const char* who)
{
    PmBuffers* b = c->pm;
    if (!b || b->maps < 1) { c->err = std::string(who) + ": no maps uploaded (drfe_plane_map_upload)"; return nullptr; }
    return b;
}

}  // namespace

int drfe_pm_run_jobs(drfe_ctx* c, PmBuffers* b, const std::vector<MpJob>& jobs, const std::vector<MpSeg>& segs, const float* poses,
                     int nposes, const float* src, size_t nsrc, hipStream_t s)
{
    return run_jobs(c, b, jobs, segs, poses, nposes, src, nsrc, s);
}

int drfe_pm_set_cloud(drfe_ctx* c, PmBuffers* b, int g, const float* xyz, int n, hipStream_t s)
{
    if (n > b->capH[g]) {
        std::vector<int64_t> need(b->cntH.size(), 0);
        need[g] = n;
        if (int rc = repack(c, b, need, s)) return rc;
    }
    if (n) HIPCHK(c, hipMemcpy(b->cloud + 3 * (size_t)b->begH[g], xyz, (size_t)n * 12, hipMemcpyHostToDevice));
    const int32_t end = b->begH[g] + n;
    HIPCHK(c, hipMemcpy(b->cloudEnd + g, &end, 4, hipMemcpyHostToDevice));
    b->cntH[g] = n;
    drfe_pm_chunks(b);
    return DRFE_OK;
}

int drfe_pm_push_planes(drfe_ctx* c, PmBuffers* b)
{
    const size_t P = b->cntH.size();
    HIPCHK(c, drfe_pm_reserve(b->mapCoefs, P * 4));
    HIPCHK(c, drfe_pm_reserve(b->mapBad, P));
    HIPCHK(c, drfe_pm_reserve(b->cloudBeg, P));
    HIPCHK(c, drfe_pm_reserve(b->cloudEnd, P));
    std::vector<int32_t> end(P);
    for (size_t j = 0; j < P; j++) end[j] = b->begH[j] + b->cntH[j];
    if (P) {
        HIPCHK(c, hipMemcpy(b->mapCoefs, b->coefsH.data(), P * 16, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(b->mapBad, b->badH.data(), P, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(b->cloudBeg, b->begH.data(), P * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(b->cloudEnd, end.data(), P * 4, hipMemcpyHostToDevice));
    }
    drfe_pm_chunks(b);
    return DRFE_OK;
}

void drfe_pm_chunks(PmBuffers* b)
{
    b->mapChunks.assign(b->maps, 0);
    for (int s = 0; s < b->maps; s++)
        for (int j = b->planeOff[s]; j < b->planeOff[s + 1]; j++) b->mapChunks[s] += (b->cntH[j] + PM_CHUNK - 1) / PM_CHUNK;
}

extern "C" {

int drfe_map_plane_update_host(const float* Tcw, const float* frame_xyz, int n_frame, const float* map_xyz, int n_map, float* out_xyz,
                               int cap, int* n_out)
{
    if (!Tcw || !n_out || n_frame < 0 || n_map < 0 || cap < 0 || (n_frame > 0 && !frame_xyz) || (n_map > 0 && !map_xyz))
        return DRFE_ERR_INVALID;
    double T[16];
    mp_pose_update(Tcw, T);
    std::vector<float> in(3 * ((size_t)n_frame + n_map));
    for (int p = 0; p < n_frame; p++)
        mp_transform_point(T, frame_xyz[3 * (size_t)p], frame_xyz[3 * (size_t)p + 1], frame_xyz[3 * (size_t)p + 2], &in[3 * (size_t)p]);
    if (n_map) std::memcpy(&in[3 * (size_t)n_frame], map_xyz, (size_t)n_map * 12);
    return finish_host(in, out_xyz, cap, n_out);
}

int drfe_map_plane_rebuild_host(int n_obs, const float* Twc, const int32_t* obs_cloud_offsets, const float* obs_xyz, float* out_xyz,
                                int cap, int* n_out)
{
    if (!n_out || n_obs < 0 || cap < 0 || (n_obs > 0 && (!Twc || !obs_cloud_offsets)) || (n_obs > 0 && !offsets_ok(obs_cloud_offsets, n_obs)) ||
        (n_obs > 0 && obs_cloud_offsets[n_obs] > obs_cloud_offsets[0] && !obs_xyz))
        return DRFE_ERR_INVALID;
    std::vector<float> in;
    if (n_obs > 0) in.resize(3 * (size_t)(obs_cloud_offsets[n_obs] - obs_cloud_offsets[0]));
    size_t at = 0;
    for (int o = 0; o < n_obs; o++) {
        double T[16];
        mp_pose_rebuild(Twc + 16 * (size_t)o, T);
        for (int p = obs_cloud_offsets[o]; p < obs_cloud_offsets[o + 1]; p++, at++)
            mp_transform_point(T, obs_xyz[3 * (size_t)p], obs_xyz[3 * (size_t)p + 1], obs_xyz[3 * (size_t)p + 2], &in[3 * at]);
    }
    return finish_host(in, out_xyz, cap, n_out);
}

int drfe_plane_map_update_batch(drfe_ctx* c, int nframes, const int32_t* frame_map, const float* Tcw, const int32_t* plane_offsets,
                                const int32_t* cloud_offsets, const float* cloud_xyz, const int32_t* map_idx, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    PmBuffers* b = maps_of(c, "plane_map_update_batch");
    if (!b) return DRFE_ERR_STATE;
    if (nframes < 1 || !frame_map || !Tcw || !plane_offsets || plane_offsets[0] != 0 || !offsets_ok(plane_offsets, nframes)) {
        c->err = "plane_map_update_batch: invalid argument";
        return DRFE_ERR_INVALID;
    }
    const int Q = plane_offsets[nframes];
    if (Q > 0 && (!cloud_offsets || !offsets_ok(cloud_offsets, Q) || (cloud_offsets[Q] > cloud_offsets[0] && !cloud_xyz))) {
        c->err = "plane_map_update_batch: invalid cloud offsets";
        return DRFE_ERR_INVALID;
    }
    for (int f = 0; f < nframes; f++)
        if (frame_map[f] < 0 || frame_map[f] >= b->maps) { c->err = "plane_map_update_batch: frame_map out of range"; return DRFE_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (b->done) HIPCHK(c, hipEventSynchronize(b->done));      /* a match batch may still read the clouds */
    std::vector<int32_t> mi((size_t)Q, -1);
    if (map_idx) {
        if (Q) std::memcpy(mi.data(), map_idx, (size_t)Q * 4);
    } else {
        /* the decisions of the most recent drfe_plane_match_batch, over the same frames */
        if (b->frames != nframes || b->frameOff != std::vector<int32_t>(plane_offsets, plane_offsets + nframes + 1) ||
            b->frameMap != std::vector<int32_t>(frame_map, frame_map + nframes)) {
            c->err = "plane_map_update_batch: map_idx NULL needs the frames of the most recent drfe_plane_match_batch";
            return DRFE_ERR_STATE;
        }
        if (Q) HIPCHK(c, hipMemcpy(mi.data(), b->io + b->offMap, (size_t)Q * 4, hipMemcpyDeviceToHost));
    }
    std::vector<Job> jobs;
    std::vector<MpSeg> segs;
    for (int f = 0; f < nframes; f++) {
        const int m = frame_map[f], M = b->planeOff[m + 1] - b->planeOff[m];
        for (int q = plane_offsets[f]; q < plane_offsets[f + 1]; q++) {
            if (mi[q] == -1) continue;
            if (mi[q] < -1 || mi[q] >= M) { c->err = "plane_map_update_batch: map_idx out of range"; return DRFE_ERR_INVALID; }
            jobs.push_back(Job{b->planeOff[m] + mi[q], (int)segs.size(), (int)segs.size() + 1, true});
            segs.push_back(MpSeg{MP_SEG_FRAME, f, cloud_offsets[q], cloud_offsets[q + 1] - cloud_offsets[q], 0, {0, 0, 0}});
        }
    }
    const size_t nsrc = Q > 0 ? (size_t)cloud_offsets[Q] : 0;
    return run_jobs(c, b, jobs, segs, Tcw, nframes, cloud_xyz, nsrc, s);
}

int drfe_plane_map_rebuild_batch(drfe_ctx* c, int njobs, const int32_t* job_map, const int32_t* job_plane, const int32_t* obs_offsets,
                                 const float* Twc, const int32_t* cloud_offsets, const float* cloud_xyz, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    PmBuffers* b = maps_of(c, "plane_map_rebuild_batch");
    if (!b) return DRFE_ERR_STATE;
    if (njobs < 1 || !job_map || !job_plane || !obs_offsets || obs_offsets[0] != 0 || !offsets_ok(obs_offsets, njobs)) {
        c->err = "plane_map_rebuild_batch: invalid argument";
        return DRFE_ERR_INVALID;
    }
    const int O = obs_offsets[njobs];
    if (O > 0 && (!Twc || !cloud_offsets || !offsets_ok(cloud_offsets, O) || (cloud_offsets[O] > cloud_offsets[0] && !cloud_xyz))) {
        c->err = "plane_map_rebuild_batch: invalid observations";
        return DRFE_ERR_INVALID;
    }
    std::vector<Job> jobs;
    std::vector<MpSeg> segs;
    for (int k = 0; k < njobs; k++) {
        const int m = job_map[k];
        if (m < 0 || m >= b->maps || job_plane[k] < 0 || job_plane[k] >= b->planeOff[m + 1] - b->planeOff[m]) {
            c->err = "plane_map_rebuild_batch: no such plane";
            return DRFE_ERR_INVALID;
        }
        jobs.push_back(Job{b->planeOff[m] + job_plane[k], (int)segs.size(), (int)segs.size() + obs_offsets[k + 1] - obs_offsets[k], false});
        for (int o = obs_offsets[k]; o < obs_offsets[k + 1]; o++)
            segs.push_back(MpSeg{MP_SEG_KEYFRAME, o, cloud_offsets[o], cloud_offsets[o + 1] - cloud_offsets[o], 0, {0, 0, 0}});
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (b->done) HIPCHK(c, hipEventSynchronize(b->done));
    const size_t nsrc = O > 0 ? (size_t)cloud_offsets[O] : 0;
    return run_jobs(c, b, jobs, segs, Twc, O, cloud_xyz, nsrc, s);
}

int drfe_plane_map_edit(drfe_ctx* c, int map, int n, const int32_t* plane_index, const float* coefs, const uint8_t* bad)
{
    if (!c) return DRFE_ERR_INVALID;
    PmBuffers* b = maps_of(c, "plane_map_edit");
    if (!b) return DRFE_ERR_STATE;
    if (map < 0 || map >= b->maps || n < 0 || (n > 0 && !plane_index) || (n > 0 && !coefs && !bad)) {
        c->err = "plane_map_edit: invalid argument";
        return DRFE_ERR_INVALID;
    }
    /* validate everything before touching the map: an appended plane needs its coefficients */
    int count = b->planeOff[map + 1] - b->planeOff[map];
    for (int k = 0; k < n; k++) {
        if (plane_index[k] < 0 || plane_index[k] > count || (plane_index[k] == count && !coefs)) {
            c->err = "plane_map_edit: plane index out of range";
            return DRFE_ERR_INVALID;
        }
        if (plane_index[k] == count) count++;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (b->done) HIPCHK(c, hipEventSynchronize(b->done));
    for (int k = 0; k < n; k++) {
        const int i = plane_index[k], g = b->planeOff[map] + i;
        if (i == b->planeOff[map + 1] - b->planeOff[map]) {          /* a new plane with an empty cloud */
            b->coefsH.insert(b->coefsH.begin() + 4 * (size_t)g, coefs + 4 * (size_t)k, coefs + 4 * (size_t)k + 4);
            b->badH.insert(b->badH.begin() + g, bad ? bad[k] : (uint8_t)0);
            b->begH.insert(b->begH.begin() + g, 0);
            b->cntH.insert(b->cntH.begin() + g, 0);
            b->capH.insert(b->capH.begin() + g, 0);
            for (int s = map + 1; s <= b->maps; s++) b->planeOff[s]++;
            continue;
        }
        if (coefs) std::memcpy(&b->coefsH[4 * (size_t)g], coefs + 4 * (size_t)k, 16);
        if (bad) b->badH[g] = bad[k];
    }
    return drfe_pm_push_planes(c, b);
}

int drfe_plane_map_cloud_download(drfe_ctx* c, int map, int plane, float* xyz, int cap, int* n)
{
    if (!c) return DRFE_ERR_INVALID;
    PmBuffers* b = maps_of(c, "plane_map_cloud_download");
    if (!b) return DRFE_ERR_STATE;
    if (!n || map < 0 || map >= b->maps || plane < 0 || plane >= b->planeOff[map + 1] - b->planeOff[map]) {
        c->err = "plane_map_cloud_download: no such plane";
        return DRFE_ERR_INVALID;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (b->done) HIPCHK(c, hipEventSynchronize(b->done));
    const int g = b->planeOff[map] + plane;
    *n = b->cntH[g];
    if (!xyz) return DRFE_OK;
    if (*n > cap) { c->err = "plane_map_cloud_download: buffer too small"; return DRFE_ERR_CAPACITY; }
    if (*n) HIPCHK(c, hipMemcpy(xyz, b->cloud + 3 * (size_t)b->begH[g], (size_t)*n * 12, hipMemcpyDeviceToHost));
    return DRFE_OK;
}

int drfe_plane_map_update_stats(drfe_ctx* c, int64_t* stats)
{
    if (!c || !stats) return DRFE_ERR_INVALID;
    PmBuffers* b = maps_of(c, "plane_map_update_stats");
    if (!b) return DRFE_ERR_STATE;
    std::memcpy(stats, b->upStats, sizeof(b->upStats));
    return DRFE_OK;
}

}  // extern "C"
