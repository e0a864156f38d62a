/* lmap_internal.h — what lmap.cpp, lmap_conn.cpp, lmap_correct.cpp, lmap_cull.cpp, lmap_gba.cpp, lmap_recent.cpp, lmap_fuse.cpp,
 * lmap_insert.cpp, lmap_create.cpp and lmap_essential.cpp hand to the store's kernels (DESIGN.md sections 25 to 29 and 31 to 35).  The host's sequence around these launches is lmap_call.h's. */
#ifndef DRFE_LMAP_INTERNAL_H
#define DRFE_LMAP_INTERNAL_H

#include "drfe_internal.h"
#include "lmap_core.h"
#include "conn_core.h"
#include "correct_core.h"
#include "cull_core.h"
#include "gba_core.h"
#include "recent_core.h"
#include "fuse_core.h"
#include "insert_core.h"
#include "create_core.h"
#include "essential_core.h"

/* threads of a workgroup: frame points and key-frame slots go across them in the vote, the entries of a match row in the gather */
#define LMAP_THREADS 256
/* stored key frames up to which a query's vote histogram is in LDS (32 KiB of the CU's 160 KiB) */
#define LMAP_LDS_KFS 8192
/* entries of one key frame's match row that a gather workgroup takes per pass */
#define LMAP_GATHER_ENTRIES LMAP_THREADS
/* gather workgroups per query: workgroup b takes the local key frames b, b + LMAP_GATHER_ROWS, ... */
#define LMAP_GATHER_ROWS 64

/* per query, written by k_lmap_vote, finished by k_lmap_scan */
struct LmapQueryRec {
    int32_t nKf, refKf;
    int32_t rec[4];
    int32_t nItems[2];             /* local points, local lines */
    int32_t nNulled, pad[3];
};

/* One chunk of a call: queries 0 .. nQ of the staged block.  Everything per (query, x) is [query * stride + x]. */
struct LmapLaunch {
    LmapImage I;                   /* resident */
    int32_t nQ;
    int32_t rowK;                  /* entries of a query's row of list / cnt: stored key frames or the longest prev_kfs list */
    int32_t rowStride[2];          /* lmap_walk_rank's stride for points, lines: above every match-row length */
    int32_t markWords;             /* (nK + 31) / 32 */
    /* per call, staged */
    const int32_t* ptOff;          /* nQ + 1, from 0 */
    const int32_t* pts;            /* point slots, -1 = null */
    const int32_t* lnOff;          /* nQ + 1 */
    const int32_t* lns;
    const int32_t* prevOff;        /* nQ + 1 */
    const int32_t* prev;           /* key-frame slots */
    /* scratch */
    int32_t* hist;                 /* nQ x nK, zero before the launch; unused while nK <= LMAP_LDS_KFS */
    uint32_t* mark;                /* nQ x markWords */
    int32_t* list;                 /* nQ x rowK: the local key frames */
    int32_t* cnt[2];               /* nQ x rowK: kept entries of each local key frame, then their exclusive prefix */
    int32_t* claim[2];             /* nQ x nP, nQ x nL: LMAP_NO_CLAIM bytes before the launch */
    uint8_t* inFrame[2];           /* nQ x nP, nQ x nL: zero before the launch */
    int32_t* nulledTmp;            /* ptOff[nQ] */
    /* out */
    LmapQueryRec* rec;             /* nQ */
    int32_t* off[4];               /* nQ + 1 each: local key frames, points, lines, nulled */
    int32_t* packedKf;             /* nQ x rowK */
    int32_t* packedItem[2];        /* nQ x nP, nQ x nL */
    uint8_t* packedIn[2];
    int32_t* packedNulled;         /* ptOff[nQ] */
};
hipError_t drfe_launch_lmap(const LmapLaunch& L, hipStream_t s);

/* ---- KeyFrame::UpdateConnections (conn_kernels.hip) ---- */
/* keys of one tile of the list sort: a workgroup ranks LMAP_THREADS keys against one tile in LDS at a time */
#define CONN_SORT_TILE LMAP_THREADS
/* workgroups of the touched-row launches: workgroup b takes the touched key frames b, b + CONN_ROW_GROUPS, ... */
#define CONN_ROW_GROUPS 256

/* the connection rows of the image, resident next to LmapImage */
struct ConnImage {
    const uint8_t* first;          /* nK: first_connection */
    const int32_t* wOff;           /* nK + 1: the weights rows, ascending slot */
    const int32_t* wKf;
    const int32_t* wW;
    const int32_t* oOff;           /* nK + 1: the ordered rows */
    const int32_t* oKf;
    const int32_t* oW;
};

/* per called key frame: counter size, listed after the fallback, nmax, pKFmax's slot or -1 */
struct ConnRec {
    int32_t nC, nL, nmax, best;
};

/* head words of a call */
enum { CONN_HEAD_TOUCHED = 0, CONN_HEAD_WEIGHTS, CONN_HEAD_ORDERED, CONN_HEAD_COUNTER, CONN_HEAD_WORDS };

/* One call.  The counter, list and edge-flag regions of called key frame p start at capOff[p]; the host sizes them from the match
 * rows (a counter has at most one entry per observation of a voting point, and at most nK - 1). */
struct ConnLaunch {
    LmapImage I;                   /* resident */
    ConnImage G;
    int32_t n;                     /* called key frames */
    int32_t chunk;                 /* called key frames per vote launch */
    /* staged */
    const int32_t* called;         /* n slots, in call order */
    const int32_t* pos;            /* nK: position in the call or -1 */
    const int32_t* capOff;         /* n + 1 */
    /* scratch */
    int32_t* hist;                 /* chunk x nK, zero before each vote launch; unused while nK <= LMAP_LDS_KFS */
    int32_t* dense;                /* CONN_ROW_GROUPS x nK; unused while nK <= LMAP_LDS_KFS */
    int32_t* cntKf;                /* capOff[n]: the counters, ascending slot */
    int32_t* cntW;
    uint64_t* lst;                 /* capOff[n]: the listed keys, descending */
    uint8_t* chg;                  /* capOff[n]: per counter entry 0 not listed, 1 AddConnection without a change, 2 with one */
    uint8_t* mark;                 /* nK, zero before the launch: touched */
    int32_t* tMode;                /* nK: per touched key frame, which list it ends with */
    /* out */
    ConnRec* rec;                  /* n */
    int32_t* newParent;            /* n: slot or -1 */
    int32_t* cntOff;               /* n + 1: offsets of the packed counters */
    int32_t* head;                 /* CONN_HEAD_WORDS */
    int32_t* touched;              /* nK: slots, ascending */
    int32_t* wOff;                 /* nK + 1: offsets of the packed final weights rows */
    int32_t* oOff;                 /* nK + 1 */
    int32_t* tParent;              /* nK: per touched key frame */
    uint8_t* tFirst;               /* nK */
    int32_t* pkCntKf;              /* capOff[n] */
    int32_t* pkCntW;
    int32_t* pkWKf;                /* the host's bound on all final weights rows */
    int32_t* pkWW;
    int32_t* pkOKf;                /* the same bound */
    int32_t* pkOW;
};
/* memsets of mark and hist, then every launch, in stream order */
hipError_t drfe_launch_conn(const ConnLaunch& L, hipStream_t s);

/* ---- LoopClosing::CorrectLoop's Sim3 propagation (correct_kernels.hip) ---- */
/* entries of a called key frame's match row that one claim workgroup takes, and one pass of a move workgroup */
#define CORRECT_TILE LMAP_THREADS
/* bytes of scratch per entry of a chunk's match rows: the packed record of a moved point (41 bytes), rounded up */
#define CORRECT_ENTRY_BYTES 48

/* One call.  Positions 0 .. n are the called key frames in rank order.  The plan launches fill kf, cnt and off for the whole call;
 * a chunk is the positions [j0, j1), whose moved points go to the packed arrays from 0 and into the image. */
struct CorrLaunch {
    LmapImage I;                   /* resident */
    CorrImage G;                   /* resident */
    int32_t n;
    int32_t cur;                   /* handle of the current key frame: the stamp */
    int32_t curPos;                /* its position */
    int32_t rowStride;             /* lmap_walk_rank's stride: above every called row length */
    int32_t maxRow;                /* the longest called row */
    int32_t j0, j1;
    double Scw[8];
    /* staged */
    const int32_t* called;         /* n slots by position */
    const int32_t* calledHandle;   /* n */
    const int32_t* pos;            /* nK: position or -1 */
    /* scratch */
    int32_t* claim;                /* nP: LMAP_NO_CLAIM bytes before the plan */
    int32_t* cnt;                  /* n: moved points of each position */
    /* out */
    CorrKf* kf;                    /* n by position */
    int32_t* off;                  /* n + 1: exclusive prefix of cnt */
    /* a chunk's packed records, in walk order */
    int32_t* pkItem;               /* point slot */
    int32_t* pkBy;                 /* claiming position */
    float* pkWorld;                /* 3 each */
    float* pkNormal;               /* 3 each */
    float* pkMax;
    float* pkMin;
    uint8_t* pkStatus;
};
/* poses of every position, the claims, the counts and their prefix */
hipError_t drfe_launch_correct_plan(const CorrLaunch& L, hipStream_t s);
/* the moved points of positions [j0, j1): packed, then scattered into the image */
hipError_t drfe_launch_correct_chunk(const CorrLaunch& L, hipStream_t s);
/* the new poses and centres into the image: after the last chunk, which still reads the stored ones */
hipError_t drfe_launch_correct_poses(const CorrLaunch& L, hipStream_t s);

/* ---- LocalMapping::KeyFrameCulling (cull_kernels.hip) ---- */
/* entries of a called key frame's match row that one record workgroup takes */
#define CULL_TILE LMAP_THREADS
/* threads of the one workgroup that walks the called key frames in order: lanes go over the entries of the key frame it is at */
#define CULL_WALK_THREADS 1024
/* bytes of scratch per entry of a chunk's match rows: its CullRecord */
#define CULL_ENTRY_BYTES 8
/* words the walk writes per called key frame: nMPs, nRedundant, action, points gone bad, observers walked (low, high) */
#define CULL_OUT_WORDS 6

/* the attributes of the image, resident in a block of their own; nObs is what the stored counters are, never written */
struct CullImage {
    const float* thDepth;          /* nK */
    const uint8_t* kfFlags;        /* nK */
    const int32_t* octave;         /* parallel to kfMp */
    const float* depth;
    const uint8_t* stereo;
    const int32_t* nObs;           /* nP */
    const int32_t* obsIdx;         /* parallel to obs */
};

/* the counts of a called key frame as the record launch found them */
struct CullSpec {
    int32_t nMPs, nRedundant;
    unsigned long long walked;
};

/* One call.  The working state is scratch: the resident image is only read.  A chunk is the positions [j0, j1) of the call, whose
 * records lie from 0 in rec, key frame after key frame (recOff). */
struct CullLaunch {
    CullState S;                   /* the working arrays in scratch, the image and the attributes resident */
    int32_t monocular;
    int32_t j0, j1;
    int32_t maxRow;                /* the longest row of the chunk */
    /* staged */
    const int32_t* called;         /* the call's slots, in call order */
    const int32_t* pos;            /* nK: position in the call or -1 */
    const int32_t* recOff;         /* one more than positions: entries of the called rows before each */
    /* scratch */
    CullRecord* rec;               /* the chunk's */
    int32_t* claim;                /* nP: 0xff bytes before the first chunk; the position whose erasure took the point last */
    uint8_t* touched;              /* nP: zero before each chunk; the point lost an observation since the chunk's records */
    CullSpec* spec;                /* per position: zero before the first chunk */
    /* out */
    int32_t* out;                  /* CULL_OUT_WORDS per position of the call */
};
/* the records of the chunk, then its walk */
hipError_t drfe_launch_cull_chunk(const CullLaunch& L, hipStream_t s);

/* ---- LocalMapping::MapPointCulling and MapLineCulling (recent_kernels.hip) ---- */
/* list entries of one workgroup of the entry launches, a lane each */
#define RECENT_TILE LMAP_THREADS
/* erased observations of one pass of an erase workgroup, a lane each, and the most workgroups of that launch */
#define RECENT_ERASE_TILE LMAP_THREADS
#define RECENT_ERASE_GROUPS 1024
/* bytes of scratch per list entry of a chunk: its observation count and its share of the workgroup totals */
#define RECENT_ENTRY_BYTES 8
/* bytes of scratch every chunk shares besides the claim words: alignment of the sections */
#define RECENT_FIXED_BYTES 1024

/* the recent-list attributes of the image, resident in a block of their own, and the line observations */
struct RecentImage {
    const int32_t* found[2];       /* nP, nL: mnFound */
    const int32_t* visible[2];     /* mnVisible */
    const int64_t* first[2];       /* mnFirstKFid */
    const int32_t* mlNObs;         /* nL: nObs as MapLine holds it */
    const int32_t* mlObsOff;       /* nL + 1 */
    const int32_t* mlObs;          /* key-frame slots */
    const int32_t* mlObsIdx;       /* parallel: mit->second */
};

/* running totals of a call, on the device across its chunks; the _BASE words are what stood there before the chunk at hand */
enum { RECENT_HEAD_KEPT_P = 0, RECENT_HEAD_KEPT_L, RECENT_HEAD_CULLED, RECENT_HEAD_ERASED,
       RECENT_HEAD_BASE, RECENT_HEAD_WORDS = 2 * RECENT_HEAD_BASE };
/* totals of one workgroup of a chunk, then their exclusive prefix over the chunk's workgroups on top of the bases */
struct RecentGroup {
    int32_t v[RECENT_HEAD_BASE];
};

/* One chunk of a call: entries [e0, e1) of the flat entry space, the nPts entries of the point list first, then the line list. */
struct RecentLaunch {
    LmapImage I;                   /* resident; the bad flags and the two kinds of match rows are written */
    CullImage A;                   /* resident: nObs and obsIdx of the points */
    RecentImage R;                 /* resident */
    int64_t current;               /* mpCurrentKeyFrame->mnId */
    int32_t monocular;
    int32_t nPts, n;               /* entries of the point list, of both lists */
    int32_t e0, e1;
    /* staged */
    const int32_t* item;           /* n slots */
    const int32_t* handle;         /* n handles, for the surviving lists */
    /* scratch */
    int32_t* claim[2];             /* nP, nL: LMAP_NO_CLAIM bytes before the first chunk */
    int32_t* cnt;                  /* per entry of the chunk: the observations its verdict erases */
    RecentGroup* group;            /* per workgroup of the chunk */
    /* out */
    uint8_t* action;               /* n */
    int32_t* kept[2];              /* the surviving lists as handles */
    int32_t* culledEntry;          /* n: the entries that carry a verdict, in list order */
    int32_t* erOff;                /* n + 1: exclusive prefix of their observation counts */
    int32_t* erKf;                 /* erased observations: key-frame slot */
    int32_t* erIdx;                /* and index */
    int32_t* head;                 /* RECENT_HEAD_WORDS, zero before the first chunk */
};
/* the claims, the verdicts, their prefix, the packed outputs with the bad flags, the erasure: in stream order.  eraseBound is the
 * host's bound on the observations the chunk erases. */
hipError_t drfe_launch_recent_chunk(const RecentLaunch& L, int64_t eraseBound, hipStream_t s);

/* ---- the fuse commit (fuse_kernels.hip) ---- */
/* candidates of one workgroup of the live pre-pass, a lane each, and the threads of the one workgroup that walks */
#define FUSE_TILE LMAP_THREADS
/* entries of the walk's append log: the observations the call added to its items so far, (item * 2 + kind, key-frame slot, index) */
#define FUSE_LOG_ENTRIES 8192
/* records the walk holds: (key-frame slot, index, moved) of every former observation of every loser */
#define FUSE_REC_ENTRIES (1 << 18)
/* stored key frames the winner's observer bitmap in LDS holds (8 KiB) */
#define FUSE_MAX_KFS 65536
/* bytes of scratch per candidate tile: its packed live candidates and their count */
#define FUSE_TILE_BYTES (4 * FUSE_TILE + 4)
/* bytes of scratch every call takes besides the per-item words: the log, the records, alignment of the sections */
#define FUSE_FIXED_BYTES (12 * FUSE_LOG_ENTRIES + 9 * FUSE_REC_ENTRIES + 1024)

struct FuseStep {
    int32_t kf, kind, form, n;
    int32_t candOff;               /* its candidates in the flat arrays */
    int32_t tile0, tile1;          /* its tiles: a step starts a tile of its own */
    int32_t pad;
};

/* head words of a call: whether the walk stopped early and where, and its totals */
enum { FUSE_HEAD_STOPPED = 0, FUSE_HEAD_STEP, FUSE_HEAD_PASS, FUSE_HEAD_CAND, FUSE_HEAD_FUSED, FUSE_HEAD_REPL, FUSE_HEAD_REC,
       FUSE_HEAD_LOG, FUSE_HEAD_WORDS };

struct FuseLaunch {
    LmapImage I;                   /* resident; the bad flags and the two kinds of match rows are written */
    CullImage A;                   /* resident: nObs of the points is written */
    RecentImage R;                 /* resident: the counters and the lines' nObs are written */
    int32_t nSteps, nTiles;
    int32_t logCap, recCap;
    /* staged */
    const FuseStep* step;          /* nSteps */
    const int32_t* tileStep;       /* nTiles: the step of each tile */
    const int32_t* cand;           /* item slots, -1 = null */
    const int32_t* best;
    /* scratch */
    int32_t* packed;               /* nTiles x FUSE_TILE: the live candidates of each tile, in order */
    int32_t* tileCnt;              /* nTiles */
    int32_t* snap;                 /* nP, zero before the launch: the LOOP step (+ 1) whose row named the point at its start */
    int32_t* clearedAt[2];         /* nP, nL, zero before the launch: 0, or 1 + the log length when a Replace last cleared the item */
    int32_t* log;                  /* 3 x logCap */
    int32_t* recKf;                /* recCap */
    int32_t* recIdx;
    uint8_t* recMoved;
    /* out */
    int32_t* head;                 /* FUSE_HEAD_WORDS */
    uint8_t* action;               /* per candidate */
    int32_t* rep;                  /* per candidate: the recorded occupant of a LOOP step (slot), else -1 */
    int32_t* nFused;               /* per step */
    int32_t* rKind;                /* per Replace, in execution order */
    int32_t* rLoser;
    int32_t* rWinner;
    int32_t* rOff;                 /* one more: offsets into the records */
};
/* the live pre-pass over every tile, then the walk: in stream order */
hipError_t drfe_launch_fuse(const FuseLaunch& L, hipStream_t s);

/* ---- the item loops of LocalMapping::ProcessNewKeyFrame (insert_kernels.hip) ---- */
/* row entries of one workgroup of the entry launches, a lane each */
#define INSERT_TILE LMAP_THREADS
/* workgroups of the normals launch at most: a lane per ADDED point entry, over a grid */
#define INSERT_NORMAL_GROUPS 1024

/* totals of a call: ADDED points, RECENT points, ADDED lines, RECENT lines */
enum { INSERT_HEAD_ADDED_P = 0, INSERT_HEAD_RECENT_P, INSERT_HEAD_ADDED_L, INSERT_HEAD_RECENT_L, INSERT_HEAD_WORDS };
/* those of one workgroup, then their exclusive prefix over the call's workgroups */
struct InsertGroup {
    int32_t v[INSERT_HEAD_WORDS];
};

/* One call.  Its rows are one flat entry space (insert_core.h): the point rows of the called key frames in call order, then their
 * line rows.  A chunk is the called key frames [j0, j1): their claim words, their verdicts and the nObs they add; the lists and the
 * records are packed once, after the last chunk. */
struct InsertLaunch {
    LmapImage I;                   /* resident */
    CullImage A;                   /* resident: nObs of the points is added to */
    RecentImage R;                 /* resident: nObs of the lines is added to */
    CorrImage G;                   /* resident; read only with normals */
    int32_t n;                     /* called key frames */
    int32_t normals;
    int32_t words;                 /* of an item's adder bits: (n + 31) / 32 */
    int32_t j0, j1;
    /* staged */
    const int32_t* called;         /* n slots, in call order */
    const int32_t* segOff;         /* 2n + 1 */
    const int32_t* byRank;         /* n: the positions of the call in ascending slot */
    const int32_t* rankOf;         /* n: the inverse */
    /* scratch */
    int32_t* claim[2];             /* (j1 - j0) x nP, (j1 - j0) x nL: LMAP_NO_CLAIM bytes before each chunk */
    uint32_t* adders;              /* nP x words, zero before the first chunk; only with normals */
    InsertGroup* group;            /* per workgroup of the flat entry space */
    int32_t* addEntry[2];          /* the ADDED entries of each kind, in walk order */
    int32_t* recent[2];            /* the RECENT items of each kind as slots, in push order */
    float* nrm;                    /* per ADDED point entry: 3 */
    float* maxD;
    float* minD;
    uint8_t* status;
    /* out */
    int32_t* head;                 /* INSERT_HEAD_WORDS */
    uint8_t* action;               /* per entry of the flat space */
};
/* the claims and the verdicts of the chunk, with the commit of nObs: in stream order after the memset of the claim words.
 * hostSegOff: segOff on the host, from which the launches size their grids */
hipError_t drfe_launch_insert_chunk(const InsertLaunch& L, const int32_t* hostSegOff, hipStream_t s);
/* after the last chunk: the totals, their prefix, the packed lists, the normals of the ADDED point entries */
hipError_t drfe_launch_insert_finish(const InsertLaunch& L, const int32_t* hostSegOff, hipStream_t s);

/* ---- map-point and map-line creation (create_kernels.hip) ---- */
/* creations of one workgroup, a lane each; the entry launches take the same number of observation entries */
#define CREATE_TILE LMAP_THREADS
/* bytes of scratch per creation of a chunk (its offset inside its tile) and per tile (the tile's observers, then their prefix) */
#define CREATE_ITEM_BYTES 4
/* bytes of scratch per stored row entry of either kind: its claim word */
#define CREATE_CLAIM_BYTES 4

/* One chunk of a call: the creations [t0, t1) of one kind.  The staged arrays hold the call's creations of that kind from 0, two
 * entries per creation where an observation is meant.  The resident sections have room behind their elements for everything the
 * call appends: the host granted it before the upload.  Creation t takes the slot slot0 + t. */
struct CreateLaunch {
    LmapImage I;                   /* resident; the bad flags, the observations and the match rows are written */
    CullImage A;                   /* resident: nObs and obsIdx of the new points are written */
    RecentImage R;                 /* resident: the counters, and all of a new line, are written */
    CorrImage G;                   /* resident: the centres and scales are read; with `geo` the new points' geometry is written */
    int32_t kind;                  /* FUSE_POINT or FUSE_LINE */
    int32_t geo, normals;
    int32_t t0, t1;
    int32_t slot0;                 /* the slot of creation 0 of the call */
    int32_t obs0;                  /* the kind's observations stored before creation t0's */
    /* staged */
    const int32_t* cnt;            /* 1 or 2 */
    const int32_t* kf;             /* 2 each: slots */
    const int32_t* idx;            /* 2 each */
    const int32_t* ref;            /* slot */
    const int64_t* first;
    const float* world;            /* 3 each; points */
    const int32_t* prev;           /* 2 each: the creation that named the same row entry last before this one, or -1 */
    /* scratch */
    int32_t* local;                /* t1 - t0: the observers of the creations before it in its tile */
    int32_t* tile;                 /* per tile of the chunk: its observers, then their exclusive prefix */
    int32_t* claim;                /* per row entry of the kind; only the words the chunk names are cleared and read */
    /* out */
    int32_t* displaced;            /* 2 each: the slot that stood in the row entry, or -1 */
    float* nrm;                    /* per point creation: 3 */
    float* maxD;
    float* minD;
    uint8_t* status;
};
/* the offsets, the claims, the new slots of every section, the row entries: in stream order */
hipError_t drfe_launch_create_chunk(const CreateLaunch& L, hipStream_t s);

/* ---- the map update of LoopClosing::RunGlobalBundleAdjustment (gba_kernels.hip) ---- */
/* point slots of one workgroup of the point launches, a lane each */
#define GBA_TILE LMAP_THREADS
/* bytes of scratch per point slot of a chunk: its kind byte, its packed record (slot, position, kind: 17 bytes) and its share of
 * the workgroup counters, rounded up */
#define GBA_POINT_BYTES 24
/* bytes of scratch every chunk shares: alignment of the sections */
#define GBA_FIXED_BYTES 1024

/* One call.  The host has walked the integer graph: list is the visited key frames in the reference's FIFO order, and the composed
 * ones among them lie round after round by their unstamped depth.  A chunk is the point slots [p0, p1). */
struct GbaLaunch {
    LmapImage I;                   /* resident */
    CorrImage G;                   /* resident */
    GbaImage B;                    /* resident */
    int32_t loop;                  /* nLoopKF as a handle: the stamp */
    int32_t nV;                    /* visited key frames */
    int32_t nRounds;               /* the deepest unstamped chain */
    int32_t p0, p1;
    int32_t pkCap;                 /* records the packed arrays hold: the host's count of the fullest chunk */
    /* staged */
    const int32_t* list;           /* nV slots */
    const int32_t* roundOff;       /* nRounds + 1 */
    const int32_t* roundKf;        /* roundOff[nRounds] slots: the composed key frames, depth 1 first */
    const int32_t* roundParent;    /* parallel: the slot of the key frame whose children row holds it */
    /* scratch, per chunk */
    uint8_t* kind;                 /* p1 - p0 */
    int32_t* groupCnt;             /* workgroups of the chunk + 1: moved points of each, then their exclusive prefix */
    int32_t* pkItem;               /* point slot */
    float* pkWorld;                /* 3 each */
    uint8_t* pkKind;
    /* out */
    float* outPose;                /* nV x 16, in list order: what SetPose received */
    float* outBef;                 /* nV x 16: mTcwBefGBA */
};
/* the composed poses round after round, then every visited key frame's commit into the two resident blocks and its record */
hipError_t drfe_launch_gba_keyframes(const GbaLaunch& L, hipStream_t s);
/* the points of the chunk: moved in place, then packed in slot order; groupCnt[workgroups] is their number */
hipError_t drfe_launch_gba_points(const GbaLaunch& L, hipStream_t s);

/* ---- what surrounds the solver of Optimizer::OptimizeEssentialGraph (essential_kernels.hip) ---- */
/* point slots of one workgroup of the commit's point launch, a lane each; edges of one workgroup of the write launch */
#define ESS_TILE LMAP_THREADS
/* lanes of the wavefront that walks one unit of the edge builder, and the wavefronts of a workgroup */
#define ESS_WAVE 64
#define ESS_WAVES (LMAP_THREADS / ESS_WAVE)
/* bytes of scratch per stored key frame of an edges call (its EssKf, its share of the unit words) and per edge of the host's bound
 * (descriptor 5 bytes, record 73 bytes, rounded up) */
#define ESS_VERTEX_BYTES 288
#define ESS_EDGE_BYTES 88
/* bytes of scratch per stored key frame of a commit call (its EssMove) and per point slot of a chunk (its record, 41 bytes,
 * rounded up) */
#define ESS_KF_BYTES 128
#define ESS_POINT_BYTES 48
/* bytes of scratch every call takes besides: alignment of the sections */
#define ESS_FIXED_BYTES 1024

/* One edges call.  Units 0 .. nLc are the rows of LoopConnections in rank order of their keys, units nLc .. nU the key frames of
 * the map (the vertices) in rank order; the descriptors of unit u lie from capOff[u], a bound the host has from the row lengths. */
struct EssEdgesLaunch {
    LmapImage I;                   /* resident */
    ConnImage C;                   /* resident */
    CorrImage G;                   /* resident: the stored poses */
    EssImage E;                    /* resident: the loop edges */
    int32_t nV, nLc, nU, nPairs;
    int32_t cur, loop;             /* slots */
    int32_t bound;                 /* capOff[nU] */
    /* staged */
    const int32_t* kfHandle;       /* nK */
    const int32_t* vert;           /* nV slots */
    const int32_t* tab;            /* nK: the key frame's row of the two tables, or -1 */
    const double* corrected;       /* 8 per row */
    const double* nonCorrected;
    const int32_t* lcKey;          /* nLc slots */
    const int32_t* lcOff;          /* nLc + 1 */
    const int32_t* lcKf;           /* member slots, ascending within a row */
    const uint64_t* pairKey;       /* nPairs: every entry as ess_pair, ascending */
    const int32_t* pairI;          /* its key */
    const int32_t* pairJ;          /* its member */
    const int32_t* capOff;         /* nU + 1 */
    /* scratch */
    EssKf* kf;                     /* nK, written for the vertices */
    int32_t* cnt;                  /* nU + 2: edges of each unit, then their exclusive prefix, the total and the emptied prefixes */
    uint8_t* emptied;              /* nU */
    int32_t* dTo;                  /* bound: the other end of each descriptor, a slot */
    uint8_t* dKind;
    /* out */
    double* outScw;                /* nV x 8 */
    int32_t* eFrom;                /* bound, filled to the total: slots */
    int32_t* eTo;
    double* eMeas;                 /* 8 each */
    uint8_t* eKind;
};
/* the vertices' Sim3s, the descriptors and counts of every unit, their prefix: in stream order */
hipError_t drfe_launch_essential_plan(const EssEdgesLaunch& L, hipStream_t s);
/* a lane per edge of the total, which the host read back after the plan */
hipError_t drfe_launch_essential_write(const EssEdgesLaunch& L, int32_t total, hipStream_t s);

/* One commit call; a chunk is the point slots [p0, p1). */
struct EssCommitLaunch {
    LmapImage I;                   /* resident */
    CorrImage G;                   /* resident: poses, centres and positions are written in place */
    int32_t n;                     /* named key frames */
    int32_t cur;                   /* handle */
    int32_t p0, p1;
    int32_t pkCap;                 /* records the packed arrays hold: the host's count of the fullest chunk */
    /* staged */
    const int32_t* named;          /* n slots, in the caller's order */
    const int32_t* posOf;          /* nK: index in the call or -1 */
    const double* scw;             /* n x 8 */
    const double* optimised;       /* n x 8 */
    const int32_t* kfHandle;       /* nK */
    const int32_t* hSorted;        /* nK: the handles ascending */
    const int32_t* hSlot;          /* nK: their slots */
    const int32_t* grpOff;         /* per workgroup of the chunk: the moved points of the chunk before it (the host's count) */
    /* scratch */
    EssMove* mv;                   /* nK */
    int32_t* pkItem;               /* point slot */
    int32_t* pkRef;                /* nIDr as a handle */
    float* pkWorld;                /* 3 each */
    float* pkNormal;               /* 3 each */
    float* pkMax;
    float* pkMin;
    uint8_t* pkStatus;
    /* out */
    float* outTiw;                 /* n x 16 */
    double* outSwc;                /* n x 8 */
};
/* a lane per stored key frame: its EssMove, and for a named one the pose and centre in place and its record */
hipError_t drfe_launch_essential_poses(const EssCommitLaunch& L, hipStream_t s);
/* the points of the chunk: moved in place, packed in slot order */
hipError_t drfe_launch_essential_points(const EssCommitLaunch& L, hipStream_t s);

#endif
