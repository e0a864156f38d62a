/* lmap_store.h — the local-map store itself: its rows by handle, the flat image of them, the optional geometry, culling attributes
 * and adjustment state by slot, and the seven resident blocks that keep them on the device (resident_block.h).  lmap_store.cpp holds
 * its lifecycle, setters, image and upload; its entries are in lmap.cpp (Tracking::UpdateLocalMap),
 * lmap_conn.cpp (KeyFrame::UpdateConnections, section 26), lmap_correct.cpp (the Sim3 propagation of LoopClosing::CorrectLoop,
 * section 27), lmap_cull.cpp (LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag, section 28), lmap_gba.cpp (the map update
 * of LoopClosing::RunGlobalBundleAdjustment, section 29), lmap_recent.cpp (LocalMapping::MapPointCulling and MapLineCulling,
 * section 31), lmap_fuse.cpp (the fuse commit with MapPoint::Replace, section 32), lmap_insert.cpp (the item loops of
 * LocalMapping::ProcessNewKeyFrame, section 33) and lmap_create.cpp (map-point and map-line creation, appended in place, section
 * 34) and lmap_essential.cpp (what surrounds the solver of Optimizer::OptimizeEssentialGraph, section 35).  What the device paths
 * share around their launches is lmap_call.h. */
#ifndef DRFE_LMAP_STORE_H
#define DRFE_LMAP_STORE_H

#include "lmap_internal.h"
#include "resident_block.h"

#include <array>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace lmap_store {

struct KfRow {
    uint64_t rank = 0;
    uint8_t bad = 0;
    int32_t parent = -1;
    int32_t nbr[LMAP_NEIGHBOURS];
    std::vector<int32_t> children, mps, mls;   /* handles */
};

/* mbFirstConnection && mnId != 0, mConnectedKeyFrameWeights and the ordered list of one key frame, by handle */
struct ConnRow {
    uint8_t first = 0;
    std::vector<int32_t> wKf, wW, oKf, oW;
};

struct MpRow {
    uint8_t bad = 0;
    std::vector<int32_t> obs;                  /* key-frame handles */
};

/* what CorrectLoop reads of a map point: GetWorldPos(), the reference key frame, its octave there and the two stamps */
struct MpGeo {
    float X[3] = {0.0f, 0.0f, 0.0f};
    int32_t ref = -1, level = 0, by = 0, byRef = 0;
};

/* the geometry by slot, next to the image; has = the item has geometry, complete = no call needs to look for a missing piece */
struct GeoImage {
    std::vector<uint8_t> kfHas, mpHas;
    std::vector<float> kfTcw, kfOw, mpWorld;
    std::vector<int32_t> mpRef, mpLevel, mpBy, mpByRef;
    bool complete = false;
};

/* what KeyFrameCulling reads of a key frame (mThDepth, the flags byte of cull_core.h, and octave, depth and stereo parallel to
 * its match row) and of a map point (nObs as the reference holds it, mit->second parallel to its observations) */
struct KfCull {
    float thDepth = 0.0f;
    uint8_t flags = 0;
    std::vector<int32_t> octave;
    std::vector<float> depth;
    std::vector<uint8_t> stereo;
};

struct MpCull {
    int32_t nObs = 0;
    std::vector<int32_t> obsIdx;
};

/* the attributes by slot, next to the image; has = the item has attributes that fit its row.  live is one flag per stored
 * observation, all set between calls: the walk clears what it erases and the commit compacts. */
struct CullAttr {
    std::vector<uint8_t> kfHas, mpHas, kfFlags, stereo, live;
    std::vector<float> thDepth, depth;
    std::vector<int32_t> octave, nObs, obsIdx;
    bool complete = false;             /* every stored item has attributes that fit and every index is inside its row */
};

/* what RunGlobalBundleAdjustment's map update reads of a key frame (mTcwGBA, mTcwBefGBA, mnBAGlobalForKF) and of a map point
 * (mPosGBA, mnBAGlobalForKF); a piece that was never given or left by a call is not there */
struct KfGba {
    float T[16] = {0}, bef[16] = {0};
    int32_t stamp = 0;
    uint8_t hasT = 0, hasBef = 0;
};

struct MpGba {
    float X[3] = {0.0f, 0.0f, 0.0f};
    int32_t stamp = 0;
    uint8_t hasX = 0;
};

/* that state by slot, next to the image; an item without state has stamp 0 and no piece */
struct GbaAttr {
    std::vector<float> kfTcwGBA, kfBef, mpPosGBA;
    std::vector<int32_t> kfStamp, mpStamp;
    std::vector<uint8_t> kfHasT, kfHasBef, mpHasPos;
};

/* what MapPointCulling and MapLineCulling read of an item (mnFound, mnVisible, mnFirstKFid), and what a map line has to hold
 * besides: nObs as MapLine holds it, its observing key frames in the caller's order and mit->second parallel to them */
struct ItemRecent {
    int32_t found = 0, visible = 0;
    int64_t first = 0;
};

struct MlObs {
    int32_t nObs = 0;
    std::vector<int32_t> obs, obsIdx;
};

/* those by slot, next to the image; has = the item has them (a point: with culling attributes that fit its observations) */
struct RecentAttr {
    std::vector<uint8_t> mpHas, mlHas;
    std::vector<int32_t> mpFound, mpVisible, mlFound, mlVisible, mlNObs, mlObsOff, mlObs, mlObsIdx;
    std::vector<int64_t> mpFirst, mlFirst;
    bool complete = false;             /* every stored point and line has them and every index is inside its observer's row */
};

/* mspLoopEdges by slot, next to the image: the known members of each row in ascending slot, and the
 * members no stored key frame answers to, which a call looks at when their edge would be added */
struct EssAttr {
    std::vector<int32_t> leOff, le;
    std::vector<std::pair<int32_t, int32_t>> unknown;   /* (key-frame slot, member handle) */
};

/* the graph with every handle resolved to a slot: what the host walk and the kernels read */
struct Image {
    std::vector<int32_t> kfHandle, mpHandle, mlHandle;   /* by slot */
    std::unordered_map<int32_t, int32_t> kfSlot, mpSlot, mlSlot;
    std::vector<uint8_t> kfBad, mpBad, mlBad;
    std::vector<int32_t> kfParent, kfNbr, childOff, child, kfMpOff, kfMp, kfMlOff, kfMl, obsOff, obs;
    int32_t maxRow[2] = {0, 0};
    /* the connection rows: weights in ascending slot, the ordered list as stored */
    std::vector<uint8_t> kfFirst;
    std::vector<int32_t> cwOff, cwKf, cwW, coOff, coKf, coW;
};

}  // namespace lmap_store

struct drfe_lmap {
    drfe_ctx* ctx = nullptr;
    int device = 0;
    std::mutex mu;
    std::string err;
    std::unordered_map<int32_t, lmap_store::KfRow> kf;
    std::unordered_map<int32_t, lmap_store::MpRow> mp;
    std::unordered_map<int32_t, uint8_t> ml;
    std::unordered_map<int32_t, lmap_store::ConnRow> conn;   /* by key-frame handle; a key frame without an entry has empty rows */
    std::unordered_map<uint64_t, int32_t> rankOwner;
    lmap_store::Image img;
    bool imgDirty = true;              /* the image lacks an edit of the rows */
    int64_t lastId = 0;
    int64_t scratchBytes = (int64_t)1 << 30;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t connStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    /* the optional geometry, by handle, and its image by slot */
    std::unordered_map<int32_t, std::array<float, 16>> kfPose;
    std::unordered_map<int32_t, lmap_store::MpGeo> mpGeo;
    std::vector<float> scales;
    lmap_store::GeoImage geo;
    bool geoDirty = true;              /* the geometry image lacks an edit of the rows or of the geometry */
    int64_t corrStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    /* the optional attributes of KeyFrameCulling, by handle, and their image by slot */
    std::unordered_map<int32_t, lmap_store::KfCull> kfCull;
    std::unordered_map<int32_t, lmap_store::MpCull> mpCull;
    lmap_store::CullAttr cull;
    bool cullDirty = true;             /* the attribute image lacks an edit of the rows or of the attributes */
    int64_t sentBytes[7] = {0, 0, 0, 0, 0, 0, 0};   /* host-to-device bytes of the rows, graph, geometry, attribute, adjustment, recent-list and loop-edge blocks */
    int64_t cullStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    /* the optional state of the map update after a global bundle adjustment, by handle, and by slot */
    std::unordered_map<int32_t, lmap_store::KfGba> kfGba;
    std::unordered_map<int32_t, lmap_store::MpGba> mpGba;
    lmap_store::GbaAttr gba;
    bool gbaDirty = true;              /* the state by slot lacks an edit of the rows or of the state */
    int64_t gbaStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    /* the optional attributes of MapPointCulling and MapLineCulling, by handle, and their image by slot */
    std::unordered_map<int32_t, lmap_store::ItemRecent> mpRec, mlRec;
    std::unordered_map<int32_t, lmap_store::MlObs> mlObs;
    lmap_store::RecentAttr rec;
    bool recDirty = true;              /* that image lacks an edit of the rows, of the culling attributes or of these */
    bool recCheck = false;             /* the line observations changed since the image looked for dangling ones */
    int64_t recStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    /* mpReplaced of the fuse commit, by handle: an item without an entry has none.  Host state only. */
    std::unordered_map<int32_t, int32_t> mpReplaced, mlReplaced;
    int64_t fuseStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t insStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};    /* of the item loops of ProcessNewKeyFrame */
    int64_t createStats[8] = {0, 0, 0, 0, 0, 0, 0, 0}; /* of map-point and map-line creation */
    /* the optional loop edges, by handle, and by slot */
    std::unordered_map<int32_t, std::vector<int32_t>> loopEdges;
    lmap_store::EssAttr ess;
    bool essDirty = true;              /* the loop edges by slot lack an edit of the rows or of the loop edges */
    int64_t essStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    /* the host walk's stamps, kept between calls: an item is stamped for the query whose serial it holds */
    std::vector<int32_t> stampP, stampL, inP, inL;
    int32_t serial = 0;
    /* the resident blocks, in upload order, with their device memory; the views of them the kernels take (d...) and the host walks
     * (h...); the sections that edits mark by name (lmap_store.cpp binds them) */
    enum { ROWS, GRAPH, GEO, ATTR, GBA, RECENT, LOOPS, BLOCKS };
    ResidentBlock blk[BLOCKS];
    DevBuf<char> dev[BLOCKS];
    LmapImage dView = {}, hView = {};
    ConnImage dConn = {};
    CorrImage dCorr = {}, hCorr = {};
    CullImage dCull = {}, hCull = {};
    GbaImage dGba = {};
    RecentImage dRec = {}, hRec = {};
    EssImage dEss = {}, hEss = {};
    int secMlBad = 0, secKfMp = 0, secKfMl = 0, secObsOff = 0, secNObs = 0, secObsIdx = 0, secRecCounters = 0, secRecObsOff = 0;
    StagePair io;
    DevBuf<char> scratch;
    PinnedBuf<char> hup, hlist;
};

/* lmap_store.cpp's: the error of a refused call; the image of the rows, rebuilt when an edit made it stale (DRFE_ERR_STATE and the
 * name of the reference when one dangles), which marks every block wholly stale: the slots may have moved */
int lmap_fail(drfe_lmap* db, int rc, const std::string& why);
int lmap_build_image(drfe_lmap* db);
/* the counts of the views and the host views' pointers, wherever the arrays are now */
void lmap_host_views(drfe_lmap* db);
/* the blocks of `need` (bit b = block b; a later block implies the rows and the graph) brought up to date in block order: the stale
 * runs staged back to back, one synchronisation.  A call's build_* runs before it. */
enum { LMAP_NEED_IMAGE = 3, LMAP_NEED_GEO = 3 | 4, LMAP_NEED_ATTR = 3 | 8, LMAP_NEED_GBA = 3 | 4 | 16, LMAP_NEED_RECENT = 3 | 8 | 32,
       LMAP_NEED_LOOPS = 3 | 4 | 64 };
int lmap_upload(drfe_lmap* db, unsigned need, hipStream_t st);
bool lmap_offsets_ok(const int32_t* off, int n);
/* lmap_correct.cpp's, for lmap_gba.cpp: the geometry by slot, rebuilt when stale */
int lmap_build_geo(drfe_lmap* db);
/* lmap_cull.cpp's, for lmap_recent.cpp: the culling attributes by slot, rebuilt when stale */
int lmap_build_cull(drfe_lmap* db);
/* lmap_recent.cpp's, for lmap_fuse.cpp: the recent-list attributes by slot, rebuilt when stale */
int lmap_build_recent(drfe_lmap* db);

#endif
