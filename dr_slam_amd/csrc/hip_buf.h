/* hip_buf.h — the host side's one HIP error check and one owning buffer type.
 *
 * HIPCHK_TO(err, call) / HIPCHK(c, call): on a failing HIP call, write "<call>: <reason>" to `err` (c->err) and return
 * DRFE_ERR_HIP from the enclosing function.
 *
 * HipBuf<T, Pinned>: a move-only device (hipMalloc) or pinned host (hipHostMalloc) array of T that frees itself.  alloc(n) frees,
 * then allocates exactly n elements; grow(n) keeps the buffer when it already holds n, else frees, then allocates n (free first:
 * the old and the new block never coexist).  A request for 0 elements allocates one.  The implicit conversion to T* lets launch
 * calls and pointer arithmetic use the buffer as the plain pointer it replaces. */
#ifndef DRFE_HIP_BUF_H
#define DRFE_HIP_BUF_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string>

#define HIPCHK_TO(err, call)                                                                    \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess) {                                                                \
            (err) = std::string(#call) + ": " + hipGetErrorString(e__);                         \
            return DRFE_ERR_HIP;                                                                \
        }                                                                                       \
    } while (0)
#define HIPCHK(c, call) HIPCHK_TO((c)->err, call)

template <class T, bool Pinned>
class HipBuf {
public:
    HipBuf() = default;
    HipBuf(const HipBuf&) = delete;
    HipBuf& operator=(const HipBuf&) = delete;
    HipBuf(HipBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    HipBuf& operator=(HipBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~HipBuf() { reset(); }

    hipError_t alloc(size_t n)
    {
        reset();
        if (!n) n = 1;
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        n_ = n;
        return hipSuccess;
    }
    hipError_t grow(size_t n) { return p_ && n_ >= n ? hipSuccess : alloc(n); }
    void reset()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }

    T* get() const { return p_; }
    size_t capacity() const { return n_; }
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;

/* StagePair: the pinned and device blocks of an entry that stages its inputs in one copy and its results in one copy back */
struct StagePair {
    PinnedBuf<char> hin, hout;
    DevBuf<char> din, dout;
    hipError_t grow(size_t in, size_t out)
    {
        hipError_t e = hin.grow(in);
        if (e == hipSuccess) e = din.grow(in);
        if (e == hipSuccess) e = hout.grow(out);
        if (e == hipSuccess) e = dout.grow(out);
        return e;
    }
};

#endif
