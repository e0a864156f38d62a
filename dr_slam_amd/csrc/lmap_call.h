/* lmap_call.h — what the device entries of the local-map store share on the host (lmap.cpp, lmap_conn.cpp, lmap_correct.cpp,
 * lmap_cull.cpp, lmap_gba.cpp, lmap_recent.cpp, lmap_fuse.cpp, lmap_insert.cpp, lmap_essential.cpp; DESIGN.md section 25, "A device call of the store"): the second-stage fetch, the
 * mark of a call that writes resident blocks, the sequence around the launches and the body of a _stats getter.  An entry keeps
 * its checks, its layout, its launch record, its chunk rule and what it does with the results.  Host only; LmapFetch and
 * LmapWrites are free of HIP, as ResidentBlock is: the copy is the caller's. */
#ifndef DRFE_LMAP_CALL_H
#define DRFE_LMAP_CALL_H

#include "lmap_store.h"

#include <assert.h>

/* Packed arrays of the scratch, at counts the device just reported, into one host block of 16-aligned sections (Fetched<T>: one
 * of them, by its element type, which gives every byte count).  add(src, n) places the next section with room for n elements and
 * asks for all of them; bytes() is the block they need.  set(n, sections...) asks for n elements of each in the same place, at
 * most what it was added with, and set(section, src, n) for n from another source: a call that runs chunk after chunk adds its
 * sections once at the fullest chunk's counts and sets every chunk's.  run(host, copy) issues copy(dst, src, bytes) for each
 * section that is not empty; at(), n() and get() then read the block. */
template <class T>
struct Fetched {
    size_t i;
};
class LmapFetch {
public:
    template <class T>
    Fetched<T> add(const T* src, size_t n)
    {
        parts_.push_back(Part{layout_.add<T>(n).off, sizeof(T), n, n, src});
        return Fetched<T>{parts_.size() - 1};
    }
    template <class... S>
    void set(size_t n, S... s) { (want(s.i, n), ...); }
    template <class T>
    void set(Fetched<T> s, const T* src, size_t n)
    {
        want(s.i, n);
        parts_[s.i].src = src;
    }
    size_t bytes() const { return layout_.bytes(); }
    template <class Copy>
    void run(char* host, Copy&& copy)
    {
        host_ = host;
        for (const Part& p : parts_)
            if (p.n) copy(host + p.off, p.src, p.n * p.elem);
    }
    template <class T>
    const T* at(Fetched<T> s) const { return reinterpret_cast<const T*>(host_ + parts_[s.i].off); }
    template <class T>
    size_t n(Fetched<T> s) const { return parts_[s.i].n; }
    template <class T>
    void get(Fetched<T> s, T* dst) const { if (n(s)) memcpy(dst, at(s), n(s) * sizeof(T)); }

private:
    struct Part {
        size_t off, elem, room, n;
        const void* src;
    };
    void want(size_t i, size_t n)
    {
        assert(n <= parts_[i].room);
        parts_[i].n = n;
    }
    StageLayout<16> layout_;
    std::vector<Part> parts_;
    char* host_ = nullptr;
};

/* A device call that writes resident blocks names them right before its first launch that writes, after everything the call can
 * be refused for: from there the host arrays are not what the device holds.  done(), after the last launch has run and with the
 * host about to commit the same values, takes the blocks as current; a call that leaves any other way leaves them to be sent
 * again by the next upload. */
struct LmapWrites {
    ResidentBlock& a;
    ResidentBlock* b;
    explicit LmapWrites(ResidentBlock& first, ResidentBlock* second = nullptr) : a(first), b(second)
    {
        a.stale_all();
        if (b) b->stale_all();
    }
    void done()
    {
        a.assume_current();
        if (b) b->assume_current();
    }
};

/* The sequence of a device call around its launches; a HIP failure in it fails the call with "<op> device call: <reason>".
 * begin: the device, the stream, the resident blocks of `need` up to date.  stage: the staging pair and the scratch grown to the
 * three layouts' bytes; `at` holds their bases from then on (the in block on the host and on the device, the out block on the
 * device, the scratch, the out block on the host).  send: the in block up, after the caller has filled it.  back takes the
 * launches' error: the out block to the host, the stream drained (drain: that alone).  fetch takes it too: the host list block
 * grown to the fetch's bytes (room: that alone, where a call lays out the fetch of all its chunks), a copy per section, the
 * stream drained.  Memsets and copies inside the scratch, and chunk loops, are the operation's own. */
struct LmapCall {
    drfe_lmap* db;
    const char* op;
    hipStream_t st = nullptr;
    size_t inBytes = 0, outBytes = 0;
    struct Bases { char* h; const char* d; char *dO, *dS; const char* ho; } at = {};

    int check(hipError_t e) const
    {
        return e == hipSuccess ? DRFE_OK : lmap_fail(db, DRFE_ERR_HIP, std::string(op) + " device call: " + hipGetErrorString(e));
    }
    int begin(unsigned need, void* stream)
    {
        if (const int rc = check(hipSetDevice(db->ctx->device))) return rc;
        st = stream ? (hipStream_t)stream : db->ctx->stream;
        return lmap_upload(db, need, st);
    }
    int stage(size_t in, size_t out, size_t scr)
    {
        hipError_t e = db->io.grow(in, out);
        if (e == hipSuccess) e = db->scratch.grow(scr);
        inBytes = in;
        outBytes = out;
        at = Bases{db->io.hin, db->io.din, db->io.dout, db->scratch, db->io.hout};
        return check(e);
    }
    int send() const { return check(hipMemcpyAsync(db->io.din, at.h, inBytes, hipMemcpyHostToDevice, st)); }
    int drain(hipError_t e) const { return check(e == hipSuccess ? hipStreamSynchronize(st) : e); }
    int back(hipError_t e) const
    {
        return drain(e == hipSuccess ? hipMemcpyAsync(db->io.hout, at.dO, outBytes, hipMemcpyDeviceToHost, st) : e);
    }
    int room(const LmapFetch& f) const { return check(db->hlist.grow(f.bytes())); }
    int fetch(LmapFetch& f, hipError_t e = hipSuccess) const
    {
        if (e == hipSuccess) e = db->hlist.grow(f.bytes());
        if (e == hipSuccess)
            f.run(db->hlist, [&](void* dst, const void* src, size_t bytes) {
                if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
            });
        return drain(e);
    }
};

/* the body of an entry's _stats */
inline int lmap_stats(drfe_lmap* db, int64_t (drfe_lmap::*counters)[8], int64_t* stats)
{
    if (!db || !stats) return DRFE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    memcpy(stats, db->*counters, sizeof(db->*counters));
    return DRFE_OK;
}

#endif
