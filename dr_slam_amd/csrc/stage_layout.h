/* stage_layout.h — how the host side divides one staging block (a pinned host block and its device twin, or the context's call
 * scratch) into typed pieces.  A piece's element type, count and place are stated once, where it is added; its byte count and its
 * pointer into either copy of the block follow from that.
 *
 * Section<T>: n elements of T at byte offset off of a block.  at(base) is the piece inside the block that starts at base (host or
 * device); put / get copy the whole piece from / to caller memory on the host (as void*: a caller's array may spell the element
 * type another way, descriptor rows as uint8_t for uint4, world coordinates as double for float).
 * StageLayout<Align>: add<T>(n) places the next section at the current end and rounds the end up to Align, so every section of a
 * block is Align-aligned; bytes() is the size of the block.  Owning the memory stays with HipBuf (hip_buf.h). */
#ifndef DRFE_STAGE_LAYOUT_H
#define DRFE_STAGE_LAYOUT_H

#include <stddef.h>
#include <string.h>

template <class T>
struct Section {
    size_t off = 0, n = 0;
    constexpr size_t bytes() const { return n * sizeof(T); }
    T* at(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
    const T* at(const void* base) const { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }
    void put(void* base, const void* src) const { if (n) memcpy(at(base), src, bytes()); }
    void get(const void* base, void* dst) const { if (n && dst) memcpy(dst, at(base), bytes()); }
};

template <size_t Align>
class StageLayout {
public:
    template <class T>
    constexpr Section<T> add(size_t n)
    {
        static_assert(Align % alignof(T) == 0, "section type over-aligned for this block");
        Section<T> s{end_, n};
        end_ = (end_ + n * sizeof(T) + Align - 1) & ~(Align - 1);
        return s;
    }
    constexpr size_t bytes() const { return end_; }

private:
    size_t end_ = 0;
};

namespace stage_layout_check {
template <size_t A>
constexpr bool offsets(size_t o1, size_t o2, size_t end)
{
    StageLayout<A> l;
    const Section<char> a = l.template add<char>(5);
    const Section<double> b = l.template add<double>(3);
    const Section<int> e = l.template add<int>(0);     /* an empty section takes no room */
    const Section<short> c = l.template add<short>(1);
    return a.off == 0 && a.bytes() == 5 && b.off == o1 && b.bytes() == 24 && e.off == o2 && e.bytes() == 0 && c.off == o2 &&
           l.bytes() == end && l.bytes() % A == 0;
}
static_assert(offsets<16>(16, 48, 64), "three sections at 16 bytes");
static_assert(offsets<64>(64, 128, 192), "three sections at 64 bytes");
static_assert(StageLayout<16>().bytes() == 0, "an empty block");
}  // namespace stage_layout_check

#endif
