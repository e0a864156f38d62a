/* plane_match.cpp — plane association (PlaneMatcher::SearchMapByCoefficients / bMatchStatus, reference
 * src/PlaneMatcher.cpp:11-226; Map::FlagMatchedPlanePoints, src/Map.cc:406-431) behind the C-ABI of include/drfe.h: the
 * single-frame host entries, the device-resident maps and the batch entry over them (plane_match_kernels.hip).  Both sides
 * evaluate plane_match_core.h; DESIGN.md section 12. */
#include "plane_map_internal.h"
#include "plane_match_core.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

bool offsets_ok(const int32_t* off, int n, int64_t total_cap = -1)
{
    if (off[0] < 0) return false;
    for (int i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    return total_cap < 0 || off[n] <= total_cap;
}

}  // namespace

void drfe_plane_match_free(drfe_ctx* c)
{
    PmBuffers* b = c->pm;
    if (!b) return;
    if (b->staged) (void)hipEventSynchronize(b->staged);
    if (b->done) (void)hipEventSynchronize(b->done);
    if (b->staged) (void)hipEventDestroy(b->staged);
    if (b->done) (void)hipEventDestroy(b->done);
    delete b;
    c->pm = nullptr;
}

extern "C" {

int drfe_plane_match_host(const drfe_plane_match_params* params, const float* Tcw, const float* coefs, int n_planes,
                          const float* map_coefs, const uint8_t* map_bad, const int32_t* cloud_offsets, const float* cloud_xyz,
                          int n_map, int32_t* map_idx, int32_t* par_idx, int32_t* ver_idx, int* nmatches)
{
    if (!params || !Tcw || !nmatches || n_planes < 0 || n_map < 0 || (n_planes > 0 && (!coefs || !map_idx || !par_idx || !ver_idx)) ||
        (n_map > 0 && (!map_coefs || !map_bad || !cloud_offsets)))
        return DRFE_ERR_INVALID;
    if (n_map > 0 && (!offsets_ok(cloud_offsets, n_map) || (cloud_offsets[n_map] > cloud_offsets[0] && !cloud_xyz)))
        return DRFE_ERR_INVALID;
    std::vector<float> angle((size_t)n_map);
    std::vector<uint32_t> key((size_t)n_map);
    int n = 0;
    for (int i = 0; i < n_planes; i++) {
        float pM[4];
        pm_world_coef(Tcw, coefs + 4 * i, pM);
        for (int j = 0; j < n_map; j++) {
            angle[j] = pm_angle(pM, map_coefs + 4 * j);
            uint32_t k = PM_NO_DISTANCE_BITS;
            if (!map_bad[j] && pm_gate(angle[j], params->aTh))
                for (int p = cloud_offsets[j]; p < cloud_offsets[j + 1]; p++)
                    k = std::min(k, pm_point_key(pM, cloud_xyz[3 * (size_t)p], cloud_xyz[3 * (size_t)p + 1], cloud_xyz[3 * (size_t)p + 2]));
            key[j] = k;
        }
        if (pm_decide(*params, angle.data(), key.data(), map_bad, n_map, map_idx + i, par_idx + i, ver_idx + i)) n++;
    }
    *nmatches = n;
    return DRFE_OK;
}

int drfe_plane_flag_points_host(const float* Tcw, const float* coefs, int n_planes, const int32_t* map_idx, const float* points_xyz,
                                int n_points, uint8_t* flags, int* n_pairs)
{
    if (!Tcw || n_planes < 0 || n_points < 0 || (n_planes > 0 && (!coefs || !map_idx)) || (n_points > 0 && (!points_xyz || !flags)))
        return DRFE_ERR_INVALID;
    int n = 0;
    for (int i = 0; i < n_planes; i++) {
        if (map_idx[i] < 0) continue;
        float pM[4];
        pm_world_coef(Tcw, coefs + 4 * i, pM);
        for (int p = 0; p < n_points; p++)
            if (pm_flag_point(pM, points_xyz[3 * (size_t)p], points_xyz[3 * (size_t)p + 1], points_xyz[3 * (size_t)p + 2])) {
                flags[p] = 1;
                n++;
            }
    }
    if (n_pairs) *n_pairs = n;
    return DRFE_OK;
}

int drfe_plane_match_status_host(const drfe_plane_match_params* params, const float* Tcw, const float* coefs, int n_planes,
                                 const float* matched_coefs, const uint8_t* matched, int MF_contrast, const float* Rwc_MF,
                                 int* status)
{
    if (!params || !Tcw || !status || n_planes < 0 || (n_planes > 0 && (!coefs || !matched_coefs || !matched)) ||
        (MF_contrast && !Rwc_MF))
        return DRFE_ERR_INVALID;
    *status = 1;
    if (n_planes < 2) return DRFE_OK;
    for (int i = 0; i < n_planes; i++) {
        if (!matched[i]) continue;
        float pM[4], pMF[4];
        pm_world_coef(Tcw, coefs + 4 * i, pM);
        const float angle = pm_angle(pM, matched_coefs + 4 * i);
        float angleMF = 0.0f;               /* uninitialised in the reference when MF_contrast is false */
        if (MF_contrast) {
            pm_world_coef_mf(Tcw, Rwc_MF, coefs + 4 * i, pMF);
            angleMF = pm_angle(pMF, matched_coefs + 4 * i);
        }
        if (pm_status_fails(angle, angleMF)) {
            *status = 0;
            return DRFE_OK;
        }
    }
    return DRFE_OK;
}

int drfe_plane_map_upload(drfe_ctx* c, int n_maps, const int32_t* plane_offsets, const float* map_coefs, const uint8_t* map_bad,
                          const int32_t* cloud_offsets, const float* cloud_xyz, const int32_t* point_offsets,
                          const float* points_xyz)
{
    if (!c) return DRFE_ERR_INVALID;
    if (n_maps < 1 || !plane_offsets || !point_offsets || plane_offsets[0] != 0 || point_offsets[0] != 0 ||
        !offsets_ok(plane_offsets, n_maps) || !offsets_ok(point_offsets, n_maps)) {
        c->err = "plane_map_upload: invalid map offsets";
        return DRFE_ERR_INVALID;
    }
    const int nPlanes = plane_offsets[n_maps];
    const size_t nPoints = (size_t)point_offsets[n_maps];
    if ((nPlanes > 0 && (!map_coefs || !map_bad || !cloud_offsets)) || (nPoints > 0 && !points_xyz)) {
        c->err = "plane_map_upload: invalid argument";
        return DRFE_ERR_INVALID;
    }
    if (nPlanes > 0 && (cloud_offsets[0] != 0 || !offsets_ok(cloud_offsets, nPlanes) || (cloud_offsets[nPlanes] > 0 && !cloud_xyz))) {
        c->err = "plane_map_upload: invalid cloud offsets";
        return DRFE_ERR_INVALID;
    }
    const size_t nCloud = nPlanes > 0 ? (size_t)cloud_offsets[nPlanes] : 0;
    HIPCHK(c, hipSetDevice(c->device));
    PmBuffers* b = c->pm;
    if (!b) { b = new PmBuffers(); c->pm = b; }
    if (b->done) HIPCHK(c, hipEventSynchronize(b->done));      /* a batch may still read the previous maps */
    HIPCHK(c, drfe_pm_reserve(b->cloud, nCloud * 3));
    HIPCHK(c, drfe_pm_reserve(b->points, nPoints * 3));
    if (nCloud) HIPCHK(c, hipMemcpy(b->cloud, cloud_xyz, nCloud * 12, hipMemcpyHostToDevice));
    if (nPoints) HIPCHK(c, hipMemcpy(b->points, points_xyz, nPoints * 12, hipMemcpyHostToDevice));
    b->maps = n_maps;
    b->planeOff.assign(plane_offsets, plane_offsets + n_maps + 1);
    b->pointOff.assign(point_offsets, point_offsets + n_maps + 1);
    b->coefsH.assign(map_coefs, map_coefs + 4 * (size_t)nPlanes);
    b->badH.assign(map_bad, map_bad + nPlanes);
    b->begH.assign(cloud_offsets, cloud_offsets + nPlanes);       /* the uploaded CSR becomes the first slot layout */
    b->cntH.resize(nPlanes);
    for (int j = 0; j < nPlanes; j++) b->cntH[j] = cloud_offsets[j + 1] - cloud_offsets[j];
    b->capH = b->cntH;
    std::fill(b->upStats, b->upStats + 4, 0);
    std::fill(b->cullStats, b->cullStats + 4, 0);
    if (int rc = drfe_pm_push_planes(c, b)) return rc;
    b->frames = 0;                    /* results of an earlier batch referred to the previous maps */
    return DRFE_OK;
}

int drfe_plane_match_batch(drfe_ctx* c, const drfe_plane_match_params* params, int nframes, const int32_t* frame_map,
                           const float* Tcw, const int32_t* plane_offsets, const float* coefs, const int32_t* map_idx,
                           const int32_t* par_idx, const int32_t* ver_idx, int flag_points, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    PmBuffers* b = c->pm;
    if (!b || b->maps < 1) { c->err = "plane_match_batch: no maps uploaded (drfe_plane_map_upload)"; return DRFE_ERR_STATE; }
    if (!params || nframes < 1 || !frame_map || !Tcw || !plane_offsets || plane_offsets[0] != 0 || !offsets_ok(plane_offsets, nframes)) {
        c->err = "plane_match_batch: invalid argument";
        return DRFE_ERR_INVALID;
    }
    const int Q = plane_offsets[nframes];
    if (Q > 0 && !coefs) { c->err = "plane_match_batch: coefs is NULL"; return DRFE_ERR_INVALID; }
    int maxPts = 0;
    int64_t workCap = 0, pairs = 0;
    for (int f = 0; f < nframes; f++) {
        const int m = frame_map[f];
        if (m < 0 || m >= b->maps) { c->err = "plane_match_batch: frame_map out of range"; return DRFE_ERR_INVALID; }
        const int P = plane_offsets[f + 1] - plane_offsets[f];
        pairs += (int64_t)P * (b->planeOff[m + 1] - b->planeOff[m]);
        workCap += (int64_t)P * b->mapChunks[m];
        if (P > 0) maxPts = std::max(maxPts, b->pointOff[m + 1] - b->pointOff[m]);
    }
    if (pairs > INT32_MAX || workCap > INT32_MAX || (int64_t)maxPts > (int64_t)PM_FLAG_POINTS * 65535) {
        c->err = "plane_match_batch: batch too large";
        return DRFE_ERR_CAPACITY;
    }
    /* packed inputs: Tcw [F x 16], coefs [Q x 4], per frame plane (frame, map, first pair) + pair total, the maps' plane and
     * point offsets, then the three index arrays (priors in, results out) */
    const size_t nOff = (size_t)b->maps + 1;
    StageLayout<16> lay;
    const auto sT = lay.add<float>((size_t)nframes * 16), sC = lay.add<float>((size_t)Q * 4);
    const auto sQ = lay.add<int32_t>((size_t)Q * 3 + 1), sO = lay.add<int32_t>(nOff * 2);
    const auto sMap = lay.add<int32_t>((size_t)Q), sPar = lay.add<int32_t>((size_t)Q), sVer = lay.add<int32_t>((size_t)Q);
    HIPCHK(c, hipSetDevice(c->device));
    if (!b->staged) HIPCHK(c, hipEventCreateWithFlags(&b->staged, hipEventDisableTiming));
    if (!b->done) HIPCHK(c, hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(b->staged));          /* the previous batch's staging is free again */
    const size_t nPoints = (size_t)b->pointOff[b->maps];
    HIPCHK(c, drfe_pm_reserve(b->hio, lay.bytes()));
    HIPCHK(c, drfe_pm_reserve(b->io, lay.bytes()));
    HIPCHK(c, drfe_pm_reserve(b->angle, (size_t)pairs));
    HIPCHK(c, drfe_pm_reserve(b->key, (size_t)pairs));
    HIPCHK(c, drfe_pm_reserve(b->work, (size_t)workCap));
    HIPCHK(c, drfe_pm_reserve(b->acc, 4 + 2 * (size_t)nframes));
    HIPCHK(c, drfe_pm_reserve(b->flags, nPoints));
    char* h = b->hio;
    sT.put(h, Tcw);
    sC.put(h, coefs);
    int32_t* qf = sQ.at(h);
    int32_t* qm = qf + Q;
    int32_t* qp = qm + Q;
    int32_t pairAt = 0;
    for (int f = 0; f < nframes; f++)
        for (int q = plane_offsets[f]; q < plane_offsets[f + 1]; q++) {
            const int m = frame_map[f];
            qf[q] = f;
            qm[q] = m;
            qp[q] = pairAt;
            pairAt += b->planeOff[m + 1] - b->planeOff[m];
        }
    qp[Q] = pairAt;
    std::memcpy(sO.at(h), b->planeOff.data(), nOff * 4);
    std::memcpy(sO.at(h) + nOff, b->pointOff.data(), nOff * 4);
    int32_t* outs[3] = {sMap.at(h), sPar.at(h), sVer.at(h)};
    const int32_t* priors[3] = {map_idx, par_idx, ver_idx};
    for (int k = 0; k < 3; k++) {
        if (priors[k]) std::memcpy(outs[k], priors[k], (size_t)Q * 4);
        else std::fill(outs[k], outs[k] + Q, -1);
    }
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, hipMemcpyAsync(b->io, b->hio, lay.bytes(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(b->staged, s));
    HIPCHK(c, hipMemsetAsync(b->acc, 0, (4 + 2 * (size_t)nframes) * 4, s));
    if (pairs) HIPCHK(c, hipMemsetAsync(b->key, 0xFF, (size_t)pairs * 4, s));
    if (flag_points && nPoints) HIPCHK(c, hipMemsetAsync(b->flags, 0, nPoints, s));
    char* d = b->io;
    PmLaunch L;
    L.Tcw = sT.at(d);
    L.coefs = sC.at(d);
    L.qFrame = sQ.at(d);
    L.qMap = L.qFrame + Q;
    L.qPair = L.qMap + Q;
    L.mapOut = sMap.at(d);
    L.parOut = sPar.at(d);
    L.verOut = sVer.at(d);
    L.planeOff = sO.at(d);
    L.pointOff = L.planeOff + nOff;
    L.mapCoefs = b->mapCoefs;
    L.mapBad = b->mapBad;
    L.cloudBeg = b->cloudBeg;
    L.cloudEnd = b->cloudEnd;
    L.cloud = b->cloud;
    L.points = b->points;
    L.angle = b->angle;
    L.key = b->key;
    L.work = b->work;
    L.workCap = (int)workCap;
    L.counter = reinterpret_cast<uint32_t*>(b->acc.get());
    L.nmatches = b->acc + 4;
    L.npairs = L.nmatches + nframes;
    L.flags = b->flags;
    L.Q = Q;
    L.maxPts = maxPts;
    L.params = *params;
    L.flagPoints = flag_points != 0;
    hipError_t e = drfe_launch_plane_match(L, s);
    if (e != hipSuccess) { c->err = std::string("plane_match_batch: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
    HIPCHK(c, hipEventRecord(b->done, s));
    b->frames = nframes;
    b->planes = Q;
    b->flagged = flag_points != 0;
    b->frameOff.assign(plane_offsets, plane_offsets + nframes + 1);
    b->frameMap.assign(frame_map, frame_map + nframes);
    b->offMap = sMap.off; b->offPar = sPar.off; b->offVer = sVer.off;
    return DRFE_OK;
}

int drfe_plane_match_download(drfe_ctx* c, int frame, int32_t* map_idx, int32_t* par_idx, int32_t* ver_idx, int* nmatches,
                              int* n_pairs)
{
    if (!c) return DRFE_ERR_INVALID;
    PmBuffers* b = c->pm;
    if (!b || frame < 0 || frame >= b->frames) { c->err = "plane_match_download: no such frame"; return DRFE_ERR_INVALID; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(b->done));
    const int q0 = b->frameOff[frame], P = b->frameOff[frame + 1] - q0;
    const char* d = b->io;
    int32_t* dst[3] = {map_idx, par_idx, ver_idx};
    const size_t off[3] = {b->offMap, b->offPar, b->offVer};
    for (int k = 0; k < 3; k++)
        if (dst[k] && P > 0) HIPCHK(c, hipMemcpy(dst[k], d + off[k] + (size_t)q0 * 4, (size_t)P * 4, hipMemcpyDeviceToHost));
    if (nmatches) HIPCHK(c, hipMemcpy(nmatches, b->acc + 4 + frame, 4, hipMemcpyDeviceToHost));
    if (n_pairs) HIPCHK(c, hipMemcpy(n_pairs, b->acc + 4 + b->frames + frame, 4, hipMemcpyDeviceToHost));
    return DRFE_OK;
}

int drfe_plane_flags_download(drfe_ctx* c, int map, uint8_t* flags)
{
    if (!c) return DRFE_ERR_INVALID;
    PmBuffers* b = c->pm;
    if (!b || b->frames < 1 || !b->flagged || map < 0 || map >= b->maps || !flags) {
        c->err = "plane_flags_download: no flags of such a map (drfe_plane_match_batch with flag_points)";
        return DRFE_ERR_INVALID;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(b->done));
    const int p0 = b->pointOff[map], n = b->pointOff[map + 1] - p0;
    if (n > 0) HIPCHK(c, hipMemcpy(flags, b->flags + p0, (size_t)n, hipMemcpyDeviceToHost));
    return DRFE_OK;
}

}  // extern "C"
