/* plane_cull.cpp — LocalMapping::MapPlaneCulling (reference src/LocalMapping.cc:233-307, Map::PointDistanceFromPlane
 * src/Map.cc:433-448, MapPlane::Replace src/MapPlane.cc:197-271) behind the C-ABI of include/drfe.h: the host entry (no context)
 * and the device entry on one resident map of drfe_plane_map_upload.  Both run the same walk over the rows (plane_cull_core.h);
 * they differ in where a pair's distance key comes from (a scan of the host cloud, or the device pass of
 * plane_cull_kernels.hip) and where a survivor's cloud is rebuilt (the host voxel grid, or the rounds of map_plane.cpp).
 *
 * Replace ends in the observation form of UpdateCoefficientsAndPoints(), a pure function of the survivor's observation set at
 * that moment, so the walk rebuilds lazily: right before the next read of that cloud as a column, right before the survivor
 * is itself replaced (its set is cleared then), or in one batch at the end of the call.  DESIGN.md section 30. */
#include "plane_map_internal.h"
#include "plane_cull_core.h"
#include "map_plane_core.h"

#include <cstring>

namespace {

const float kLeaf = 0.05f;

bool offsets_ok(const int32_t* off, int n)
{
    if (off[0] != 0) return false;
    for (int i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    return true;
}

const char* validate(const drfe_plane_cull_in* in, const drfe_plane_cull_out* out)
{
    if (!in || !out) return "NULL argument";
    const int P = in->n_planes;
    if (P < 0 || in->n_kfs < 0 || in->n_recent < 0) return "negative count";
    if (P > 0 && (!in->found || !in->visible || !in->n_obs || !in->first_kf_id || !in->obs_offsets)) return "NULL plane array";
    if (P > 0 && (!out->events || !out->bad || !out->n_obs || !out->found || !out->visible || !out->rebuilt || !out->rebuilt_offsets))
        return "NULL output array";
    if (in->n_recent > 0 && (!in->recent || !out->verdicts)) return "NULL recent list";
    if (out->rebuilt_capacity < 0 || (out->rebuilt_capacity > 0 && !out->rebuilt_xyz)) return "invalid rebuilt capacity";
    if (P > 0 && !offsets_ok(in->obs_offsets, P)) return "invalid observation offsets";
    const int O = P > 0 ? in->obs_offsets[P] : 0;
    if (O > 0 && (!in->obs_kf || !in->obs_idx || !in->obs_cloud || !in->obs_cloud_n || !in->Twc)) return "NULL observation array";
    if (O > 0 && (in->obs_cloud_stride < 12 || in->obs_cloud_stride % 4)) return "invalid cloud stride";
    for (int p = 0; p < P; p++)
        for (int o = in->obs_offsets[p]; o < in->obs_offsets[p + 1]; o++) {
            if (in->obs_kf[o] < 0 || in->obs_kf[o] >= in->n_kfs) return "observation key frame out of range";
            if (o > in->obs_offsets[p] && in->obs_kf[o] <= in->obs_kf[o - 1]) return "observations not in key-frame order";
            if (in->obs_cloud_n[o] < 0 || (in->obs_cloud_n[o] > 0 && !in->obs_cloud[o])) return "invalid observation cloud";
        }
    for (int k = 0; k < in->n_recent; k++)
        if (in->recent[k] < -1 || in->recent[k] >= P) return "recent index out of range";
    return nullptr;
}

struct Walk;

/* where keys come from and where clouds are rebuilt */
struct Backend {
    virtual ~Backend() {}
    virtual float angle(int i, int j) = 0;
    virtual int points(int j) = 0;                       /* the current size of plane j's cloud */
    virtual uint32_t key(int i, int j) = 0;              /* min pc_point_key of plane j's current cloud against plane i */
    /* rebuilds the clouds of `planes` from their current observation sets; row >= 0: the one plane is about to be read as a
     * column by rows row, row + 1, ... */
    virtual int rebuild(const Walk& w, const std::vector<int>& planes, int row) = 0;
    virtual int cloud(int j, std::vector<float>& xyz) = 0;
};

struct Walk {
    const drfe_plane_cull_in* in;
    int P;
    std::vector<uint8_t> bad, pending, rebuilt;
    std::vector<int32_t> nobs, found, visible;
    std::vector<std::vector<int32_t>> okf, oidx, oobs;   /* per plane: key-frame rank, plane in the key frame, input observation */
    std::vector<int32_t> events;
    int64_t counters[4] = {0, 0, 0, 0};

    Walk(const drfe_plane_cull_in* in_, const uint8_t* bad0) : in(in_), P(in_->n_planes)
    {
        bad.assign(bad0, bad0 + P);
        pending.assign(P, 0);
        rebuilt.assign(P, 0);
        nobs.assign(in->n_obs, in->n_obs + P);
        found.assign(in->found, in->found + P);
        visible.assign(in->visible, in->visible + P);
        okf.resize(P); oidx.resize(P); oobs.resize(P);
        for (int p = 0; p < P; p++)
            for (int o = in->obs_offsets[p]; o < in->obs_offsets[p + 1]; o++) {
                okf[p].push_back(in->obs_kf[o]);
                oidx[p].push_back(in->obs_idx[o]);
                oobs[p].push_back(o);
            }
    }

    int flush(Backend& be, int j, int row)
    {
        if (!pending[j]) return DRFE_OK;
        pending[j] = 0;
        counters[2]++;
        if (row >= 0) counters[3]++;
        return be.rebuild(*this, std::vector<int>(1, j), row);
    }

    /* Replace (:197-271): the survivor takes the replaced plane's observations, found and visible; the rebuild is deferred */
    int replace(Backend& be, int dead, int surv)
    {
        if (int rc = flush(be, dead, -1)) return rc;       /* its set is cleared below: the cloud it was left with */
        const int nd = (int)okf[dead].size(), ns = (int)okf[surv].size();
        std::vector<int32_t> mk(nd + ns), mi(nd + ns), mo;
        int added = 0;
        const int n = pc_merge_observations(okf[dead].data(), oidx[dead].data(), nd, okf[surv].data(), oidx[surv].data(), ns, mk.data(),
                                            mi.data(), &added);
        /* the input observation behind every merged entry, by the same walk */
        for (int k = 0, a = 0, b = 0; k < n; k++) {
            if (b < ns && mk[k] == okf[surv][b]) {
                mo.push_back(oobs[surv][b++]);
                if (a < nd && okf[dead][a] == mk[k]) a++;
            } else
                mo.push_back(oobs[dead][a++]);
        }
        mk.resize(n); mi.resize(n);
        okf[surv].swap(mk); oidx[surv].swap(mi); oobs[surv].swap(mo);
        okf[dead].clear(); oidx[dead].clear(); oobs[dead].clear();
        bad[dead] = 1;
        nobs[surv] += added;
        found[surv] += found[dead];
        visible[surv] += visible[dead];
        pending[surv] = 1;
        rebuilt[surv] = 1;
        events.push_back(dead);
        events.push_back(surv);
        return DRFE_OK;
    }

    int run(Backend& be)
    {
        std::vector<float> ang((size_t)P);
        std::vector<uint32_t> key((size_t)P);
        for (int i = 0; i < P; i++) {
            if (bad[i]) continue;
            for (int j = i + 1; j < P; j++) {
                ang[j] = be.angle(i, j);
                key[j] = PM_NO_DISTANCE_BITS;
                if (bad[j] || !pc_gate(ang[j], in->aTh)) continue;
                if (int rc = flush(be, j, i)) return rc;
                counters[0]++;
                counters[1] += be.points(j);
                key[j] = be.key(i, j);
            }
            const int best = pc_decide_row(in->dTh, in->aTh, ang.data(), key.data(), bad.data(), i, P);
            if (best < 0) continue;
            /* Replace with equal mnId returns at once; it cannot happen for i < best over distinct planes */
            const bool first = pc_first_survives(nobs[i], nobs[best]);
            if (int rc = replace(be, first ? best : i, first ? i : best)) return rc;
        }
        std::vector<int> rest;
        for (int j = 0; j < P; j++)
            if (pending[j]) { rest.push_back(j); pending[j] = 0; }
        counters[2] += (int64_t)rest.size();
        if (!rest.empty())
            if (int rc = be.rebuild(*this, rest, -1)) return rc;
        return DRFE_OK;
    }

    /* the recent list (:278-306) and the outputs */
    int finish(Backend& be, drfe_plane_cull_out* out)
    {
        for (int k = 0; k < in->n_recent; k++) {
            const int p = in->recent[k];
            const int v = p < 0 ? (int)DRFE_PLANE_CULL_ERASED_BAD
                                : pc_recent_verdict(bad[p] != 0, found[p], visible[p], nobs[p], in->first_kf_id[p], in->current_kf_id);
            if (v == DRFE_PLANE_CULL_BAD_BY_RATIO || v == DRFE_PLANE_CULL_BAD_BY_OBSERVATIONS) bad[p] = 1;
            out->verdicts[k] = (uint8_t)v;
        }
        out->n_events = (int32_t)(events.size() / 2);
        if (!events.empty()) std::memcpy(out->events, events.data(), events.size() * 4);
        if (P) {
            std::memcpy(out->bad, bad.data(), (size_t)P);
            std::memcpy(out->n_obs, nobs.data(), (size_t)P * 4);
            std::memcpy(out->found, found.data(), (size_t)P * 4);
            std::memcpy(out->visible, visible.data(), (size_t)P * 4);
        }
        std::memcpy(out->counters, counters, sizeof(counters));
        int nr = 0;
        int64_t at = 0;
        std::vector<float> xyz;
        if (P) out->rebuilt_offsets[0] = 0;
        int rc = DRFE_OK;
        for (int j = 0; j < P; j++) {
            if (!rebuilt[j]) continue;
            if (int e = be.cloud(j, xyz)) return e;
            const int64_t m = (int64_t)(xyz.size() / 3);
            if (at + m > out->rebuilt_capacity) rc = DRFE_ERR_CAPACITY;
            if (rc == DRFE_OK && m) std::memcpy(out->rebuilt_xyz + 3 * at, xyz.data(), (size_t)m * 12);
            if (rc == DRFE_OK) at += m;
            out->rebuilt[nr++] = j;
            out->rebuilt_offsets[nr] = (int32_t)at;
        }
        out->n_rebuilt = nr;
        return rc;
    }
};

const float* obs_point(const drfe_plane_cull_in* in, int o, int q)
{
    return reinterpret_cast<const float*>(reinterpret_cast<const char*>(in->obs_cloud[o]) + (size_t)q * in->obs_cloud_stride);
}

/* the observation form on the host: every observation's cloud moved by its Twc, in set order, then the voxel grid */
int rebuild_host(const Walk& w, int j, std::vector<float>& out)
{
    const drfe_plane_cull_in* in = w.in;
    size_t total = 0;
    for (int o : w.oobs[j]) total += (size_t)in->obs_cloud_n[o];
    if (total > INT32_MAX) return DRFE_ERR_CAPACITY;
    std::vector<float> comb(3 * total);
    size_t at = 0;
    for (size_t k = 0; k < w.oobs[j].size(); k++) {
        const int o = w.oobs[j][k];
        double T[16];
        mp_pose_rebuild(in->Twc + 16 * (size_t)w.okf[j][k], T);
        for (int q = 0; q < in->obs_cloud_n[o]; q++, at++) {
            const float* p = obs_point(in, o, q);
            mp_transform_point(T, p[0], p[1], p[2], &comb[3 * at]);
        }
    }
    static const float none[3] = {0.f, 0.f, 0.f};
    out.resize(std::max<size_t>(3 * total, 3));
    int m = 0;
    const int rc = drfe_plane_voxel_grid(total ? comb.data() : none, (int)total, kLeaf, out.data(), (int)total, &m);
    out.resize(3 * (size_t)std::max(m, 0));
    return rc;
}

/* the reference's walk as written: a pair's key is a scan of plane j's cloud */
struct HostBackend : Backend {
    const float* coefs;
    std::vector<const float*> ptr;               /* the caller's cloud until the plane is rebuilt */
    std::vector<int32_t> cnt;
    std::vector<std::vector<float>> own;

    HostBackend(int P, const float* coefs_, const int32_t* off, const float* xyz) : coefs(coefs_), ptr(P), cnt(P), own(P)
    {
        for (int j = 0; j < P; j++) {
            ptr[j] = xyz ? xyz + 3 * (size_t)off[j] : nullptr;
            cnt[j] = off[j + 1] - off[j];
        }
    }
    float angle(int i, int j) override { return pm_angle(coefs + 4 * (size_t)i, coefs + 4 * (size_t)j); }
    int points(int j) override { return cnt[j]; }
    uint32_t key(int i, int j) override
    {
        uint32_t k = PM_NO_DISTANCE_BITS;
        const float* p = ptr[j];
        for (int q = 0; q < cnt[j]; q++) k = std::min(k, pc_point_key(coefs + 4 * (size_t)i, p[3 * (size_t)q], p[3 * (size_t)q + 1], p[3 * (size_t)q + 2]));
        return k;
    }
    int rebuild(const Walk& w, const std::vector<int>& planes, int) override
    {
        for (int j : planes) {
            if (int rc = rebuild_host(w, j, own[j])) return rc;
            ptr[j] = own[j].data();
            cnt[j] = (int32_t)(own[j].size() / 3);
        }
        return DRFE_OK;
    }
    int cloud(int j, std::vector<float>& xyz) override
    {
        xyz.assign(ptr[j], ptr[j] + 3 * (size_t)cnt[j]);
        return DRFE_OK;
    }
};

/* keys from the device pass over the resident clouds, rebuilds through the rounds of map_plane.cpp */
struct DeviceBackend : Backend {
    drfe_ctx* c;
    PmBuffers* b;
    hipStream_t s;
    PcLaunch L;
    std::vector<float> ang;
    std::vector<uint32_t> keys;

    float angle(int i, int j) override { return ang[pc_pair_index(i, j)]; }
    int points(int j) override { return b->cntH[L.pb + j]; }
    uint32_t key(int i, int j) override { return keys[pc_pair_index(i, j)]; }

    int first_pass()
    {
        const int P = L.P;
        const size_t T = (size_t)P * (P - 1) / 2;
        HIPCHK(c, drfe_pm_reserve(b->pcAngle, T));
        HIPCHK(c, drfe_pm_reserve(b->pcKey, T));
        HIPCHK(c, drfe_pm_reserve(b->pcRowList, T));
        HIPCHK(c, drfe_pm_reserve(b->pcRowCount, (size_t)P));
        L.angle = b->pcAngle; L.key = b->pcKey; L.rowList = b->pcRowList; L.rowCount = b->pcRowCount;
        ang.assign(T, 0.f);
        keys.assign(T, PM_NO_DISTANCE_BITS);
        if (P < 2) return DRFE_OK;
        int maxN = 0;
        for (int j = 1; j < P; j++) maxN = std::max(maxN, b->cntH[L.pb + j]);
        HIPCHK(c, hipMemsetAsync(b->pcRowCount, 0, (size_t)P * 4, s));
        hipError_t e = drfe_launch_plane_cull_pairs(L, s);
        if (e == hipSuccess) e = drfe_launch_plane_cull_dist(L, 1, P - 1, (maxN + PC_CHUNK - 1) / PC_CHUNK, P - 1, s);
        if (e != hipSuccess) { c->err = std::string("plane_map_cull: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
        HIPCHK(c, hipMemcpyAsync(ang.data(), b->pcAngle, T * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(keys.data(), b->pcKey, T * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        b->cullStats[2]++;
        return DRFE_OK;
    }

    /* column j again, over its rebuilt cloud, for the rows row .. j - 1 that can still read it */
    int recompute(const Walk& w, int j, int row)
    {
        std::vector<int32_t> rows;
        const int n = b->cntH[L.pb + j];
        if (n > 0)
            for (int i = row; i < j; i++)
                if (!w.bad[i] && pc_gate(angle(i, j), w.in->aTh)) rows.push_back(i);
        const int at = pc_pair_index(0, j), nr = (int)rows.size();
        std::fill(keys.begin() + at, keys.begin() + at + j, PM_NO_DISTANCE_BITS);
        if (nr == 0) return DRFE_OK;
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(b->pcKey + at), (int)PM_NO_DISTANCE_BITS, (size_t)j, s));
        HIPCHK(c, hipMemcpyAsync(b->pcRowList + at, rows.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(b->pcRowCount + j, &nr, 4, hipMemcpyHostToDevice, s));
        hipError_t e = drfe_launch_plane_cull_dist(L, j, 1, (n + PC_CHUNK - 1) / PC_CHUNK, nr, s);
        if (e != hipSuccess) { c->err = std::string("plane_map_cull: ") + hipGetErrorString(e); return DRFE_ERR_HIP; }
        HIPCHK(c, hipMemcpyAsync(keys.data() + at, b->pcKey + at, (size_t)j * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));              /* rows and nr are read by the copies until here */
        b->cullStats[2]++;
        return DRFE_OK;
    }

    int rebuild(const Walk& w, const std::vector<int>& planes, int row) override
    {
        const drfe_plane_cull_in* in = w.in;
        std::vector<MpJob> jobs;
        std::vector<MpSeg> segs;
        std::vector<float> src;
        for (int j : planes) {
            jobs.push_back(MpJob{L.pb + j, (int)segs.size(), (int)(segs.size() + w.oobs[j].size()), false});
            for (size_t k = 0; k < w.oobs[j].size(); k++) {
                const int o = w.oobs[j][k], n = in->obs_cloud_n[o];
                if (src.size() / 3 + (size_t)n > INT32_MAX) { c->err = "plane_map_cull: a rebuild outgrows 2^31 points"; return DRFE_ERR_CAPACITY; }
                segs.push_back(MpSeg{MP_SEG_KEYFRAME, w.okf[j][k], (int32_t)(src.size() / 3), n, 0, {0, 0, 0}});
                for (int q = 0; q < n; q++) {
                    const float* p = obs_point(in, o, q);
                    src.insert(src.end(), p, p + 3);
                }
            }
        }
        if (int rc = drfe_pm_run_jobs(c, b, jobs, segs, in->Twc, in->n_kfs, src.data(), src.size() / 3, s)) return rc;
        b->cullStats[3]++;
        /* a repack moves the arena and the per-plane arrays */
        L.mapCoefs = b->mapCoefs; L.mapBad = b->mapBad; L.cloud = b->cloud; L.cloudBeg = b->cloudBeg; L.cloudEnd = b->cloudEnd;
        return row >= 0 ? recompute(w, planes[0], row) : DRFE_OK;
    }

    int cloud(int j, std::vector<float>& xyz) override
    {
        const int g = L.pb + j, n = b->cntH[g];
        xyz.resize(3 * (size_t)n);
        if (n) HIPCHK(c, hipMemcpy(xyz.data(), b->cloud + 3 * (size_t)b->begH[g], (size_t)n * 12, hipMemcpyDeviceToHost));
        return DRFE_OK;
    }
};

}  // namespace

extern "C" {

int drfe_plane_map_cull_host(const drfe_plane_cull_in* in, const float* map_coefs, const uint8_t* map_bad, const int32_t* cloud_offsets,
                             const float* cloud_xyz, drfe_plane_cull_out* out)
{
    if (validate(in, out)) return DRFE_ERR_INVALID;
    const int P = in->n_planes;
    if (P > 0 && (!map_coefs || !map_bad || !cloud_offsets || !offsets_ok(cloud_offsets, P) || (cloud_offsets[P] > 0 && !cloud_xyz)))
        return DRFE_ERR_INVALID;
    static const uint8_t none = 0;
    Walk w(in, P ? map_bad : &none);
    HostBackend be(P, map_coefs, cloud_offsets, cloud_xyz);
    if (int rc = w.run(be)) return rc;
    return w.finish(be, out);
}

int drfe_plane_map_cull_batch(drfe_ctx* c, int map, const drfe_plane_cull_in* in, int mode, drfe_plane_cull_out* out, void* stream)
{
    if (!c) return DRFE_ERR_INVALID;
    PmBuffers* b = c->pm;
    if (!b || b->maps < 1) { c->err = "plane_map_cull_batch: no maps uploaded (drfe_plane_map_upload)"; return DRFE_ERR_STATE; }
    if (const char* why = validate(in, out)) { c->err = std::string("plane_map_cull_batch: ") + why; return DRFE_ERR_INVALID; }
    if (map < 0 || map >= b->maps || mode < 0 || mode > 3) { c->err = "plane_map_cull_batch: no such map or mode"; return DRFE_ERR_INVALID; }
    const int pb = b->planeOff[map], P = b->planeOff[map + 1] - pb;
    if (in->n_planes != P) { c->err = "plane_map_cull_batch: n_planes is not the resident map's plane count"; return DRFE_ERR_STATE; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (b->done) HIPCHK(c, hipEventSynchronize(b->done));      /* a match batch may still read the clouds */
    int maxN = 0;
    for (int j = 0; j < P; j++) maxN = std::max(maxN, b->cntH[pb + j]);
    const int tile = mode == 3 ? 1 : PC_ROW_TILE;
    bool device = mode == 1 || mode == 3 || (mode == 0 && P >= DRFE_PLANE_CULL_DEVICE_FROM);
    /* the distance pass is one grid of (chunks, columns, row tiles) */
    if (P > DRFE_PLANE_CULL_MAX_PLANES || (int64_t)((maxN + PC_CHUNK - 1) / PC_CHUNK) * P * ((P + tile - 1) / tile) > INT32_MAX) device = false;
    b->cullStats[0]++;
    static const uint8_t none = 0;
    Walk w(in, P ? &b->badH[pb] : &none);
    int rc;
    if (device) {
        b->cullStats[1]++;
        DeviceBackend be;
        be.c = c; be.b = b; be.s = s;
        be.L = PcLaunch{b->mapCoefs, b->cloud, b->mapBad, b->cloudBeg, b->cloudEnd, nullptr, nullptr, nullptr, nullptr, pb, P, tile, in->aTh};
        if ((rc = be.first_pass())) return rc;
        if ((rc = w.run(be))) return rc;
        rc = w.finish(be, out);
    } else {
        /* the host walk over the downloaded clouds; the rebuilt clouds go back into their slots */
        std::vector<int32_t> off((size_t)P + 1, 0);
        for (int j = 0; j < P; j++) off[j + 1] = off[j] + b->cntH[pb + j];
        std::vector<float> xyz(3 * (size_t)off[P] + 3);
        for (int j = 0; j < P; j++)
            if (b->cntH[pb + j])
                HIPCHK(c, hipMemcpy(&xyz[3 * (size_t)off[j]], b->cloud + 3 * (size_t)b->begH[pb + j], (size_t)b->cntH[pb + j] * 12, hipMemcpyDeviceToHost));
        HostBackend be(P, P ? &b->coefsH[4 * (size_t)pb] : nullptr, off.data(), xyz.data());
        if ((rc = w.run(be))) { c->err = "plane_map_cull_batch: the host walk failed"; return rc; }
        rc = w.finish(be, out);
        for (int j = 0; j < P; j++)
            if (w.rebuilt[j])
                if (int e = drfe_pm_set_cloud(c, b, pb + j, be.ptr[j], be.cnt[j], s)) return e;
    }
    if (rc != DRFE_OK && rc != DRFE_ERR_CAPACITY) return rc;
    if (rc == DRFE_ERR_CAPACITY) c->err = "plane_map_cull_batch: rebuilt_capacity too small";
    /* the bad flags: the merges and the list verdicts (w.bad holds both after finish) */
    if (P && std::memcmp(&b->badH[pb], w.bad.data(), (size_t)P)) {
        std::memcpy(&b->badH[pb], w.bad.data(), (size_t)P);
        HIPCHK(c, hipMemcpy(b->mapBad + pb, w.bad.data(), (size_t)P, hipMemcpyHostToDevice));
    }
    return rc;
}

int drfe_plane_map_cull_limits(int32_t* out4)
{
    if (!out4) return DRFE_ERR_INVALID;
    out4[0] = PC_CHUNK;
    out4[1] = PC_ROW_TILE;
    out4[2] = DRFE_PLANE_CULL_DEVICE_FROM;
    out4[3] = DRFE_PLANE_CULL_MAX_PLANES;
    return DRFE_OK;
}

int drfe_plane_map_cull_stats(drfe_ctx* c, int64_t* stats)
{
    if (!c || !stats) return DRFE_ERR_INVALID;
    PmBuffers* b = c->pm;
    if (!b || b->maps < 1) { c->err = "plane_map_cull_stats: no maps uploaded (drfe_plane_map_upload)"; return DRFE_ERR_STATE; }
    std::memcpy(stats, b->cullStats, sizeof(b->cullStats));
    return DRFE_OK;
}

}  // extern "C"
