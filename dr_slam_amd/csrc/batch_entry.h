/* batch_entry.h — what the batch entries that stage a call in one block each way share on the host (the RANSAC solvers sim3.cpp,
 * pnp.cpp, init.cpp and the optimisers pose_opt.cpp, trans_opt.cpp, sim3_opt.cpp): the buffers an entry keeps in the context,
 * their counters and hand-back switch, and the sequence around the launch that does not depend on the mathematics:
 *   batch_begin    set the device, pick the stream, grow the blocks; the caller then fills io.hin
 *   batch_upload   the copy to the device, the out block zeroed; the caller then launches
 *   batch_finish   the launches' error, the out block back to the host, the stream drained (batch_copy_back without the drain)
 * An entry keeps its argument checks, its records, its layout and what it does with the results.  Host only. */
#ifndef DRFE_BATCH_ENTRY_H
#define DRFE_BATCH_ENTRY_H

#include "drfe_internal.h"

#include <cstring>
#include <string>

/* an entry's buffers in the context */
struct BatchBuffers {
    StagePair io;                      /* staging: one copy each way */
    DevBuf<char> scratch;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int handBackEvery = 0;             /* an entry's debug hand-back hook: treat every k-th unit of a call as not certified */
};

/* the entry's buffers, made at its first call */
template <class B>
B* batch_buffers(B*& slot)
{
    if (!slot) slot = new B();
    return slot;
}

template <class B>
void batch_free(B*& slot)
{
    delete slot;
    slot = nullptr;
}

/* the body of an entry's _stats: zeros before its first call */
template <class B>
int batch_stats(drfe_ctx* c, B* drfe_ctx::*slot, int64_t* stats)
{
    if (!c || !stats) return DRFE_ERR_INVALID;
    const BatchBuffers* b = c->*slot;
    if (b) std::memcpy(stats, b->stats, sizeof(b->stats));
    else std::memset(stats, 0, 8 * sizeof(int64_t));
    return DRFE_OK;
}

/* the body of an entry's _debug_*_hand_back */
template <class B>
int batch_hand_back(drfe_ctx* c, B* drfe_ctx::*slot, int every)
{
    if (!c || every < 0) return DRFE_ERR_INVALID;
    batch_buffers(c->*slot)->handBackEvery = every;
    return DRFE_OK;
}

/* a check of one offsets table of a call of n frames: starts at 0, does not decrease, no frame above cap (named capName) */
inline bool batch_offsets_ok(const char* name, const int32_t* off, int n, int cap, const char* what, const char* capName, std::string& err)
{
    if (off[0] != 0) { err = std::string(name) + ": " + what + "_offsets[0] is not 0"; return false; }
    for (int f = 0; f < n; f++) {
        if (off[f + 1] < off[f]) { err = std::string(name) + ": decreasing " + what + "_offsets"; return false; }
        if (off[f + 1] - off[f] > cap) { err = std::string(name) + ": more than " + capName + " in a frame"; return false; }
    }
    return true;
}

inline int batch_begin(drfe_ctx* c, BatchBuffers* b, void* stream, size_t inBytes, size_t outBytes, size_t scratchBytes, hipStream_t* st)
{
    HIPCHK(c, hipSetDevice(c->device));
    *st = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, b->io.grow(inBytes, outBytes));
    HIPCHK(c, b->scratch.grow(scratchBytes));
    return DRFE_OK;
}

/* zeroBytes of the out block are cleared: all of it, or 0 for an entry whose kernels write every byte they return */
inline int batch_upload(drfe_ctx* c, BatchBuffers* b, size_t inBytes, size_t zeroBytes, hipStream_t st)
{
    HIPCHK(c, hipMemcpyAsync(b->io.din, b->io.hin, inBytes, hipMemcpyHostToDevice, st));
    if (zeroBytes) HIPCHK(c, hipMemsetAsync(b->io.dout, 0, zeroBytes, st));
    return DRFE_OK;
}

inline int batch_copy_back(drfe_ctx* c, const char* name, hipError_t e, BatchBuffers* b, size_t outBytes, hipStream_t st)
{
    if (e == hipSuccess) e = hipMemcpyAsync(b->io.hout, b->io.dout, outBytes, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) { c->err = std::string(name) + " batch: " + hipGetErrorString(e); return DRFE_ERR_HIP; }
    return DRFE_OK;
}

inline int batch_finish(drfe_ctx* c, const char* name, hipError_t e, BatchBuffers* b, size_t outBytes, hipStream_t st)
{
    if (const int rc = batch_copy_back(c, name, e, b, outBytes, st)) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return DRFE_OK;
}

#endif
