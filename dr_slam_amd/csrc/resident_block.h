/* resident_block.h — one block of host arrays kept current on the device, on top of StageLayout (stage_layout.h); the memory on
 * either side stays with HipBuf (hip_buf.h).  Host-only, and free of HIP: the copy is the caller's.
 *
 * A block is an ordered list of bindings, one line per array: the std::vector that holds it (the object, not its data(): contents
 * are swapped and reassigned), the field of the device view that points at it and, optionally, the field of the host view.  The
 * layout (sections in binding order, each 16-aligned), the pack into staging, both views and the byte count follow from the list.
 *
 * Per section the block remembers the offset and byte count the device copy holds, and a stale mark: stale(first, last),
 * stale_all(), stale_at(section, index) for one element, assume_current() after a device call that wrote the block itself while
 * the host arrays were committed to the same values.  plan(have) lays the arrays out at their current sizes; a section goes up
 * when it is marked, when its offset or size is not what the device holds, or when the block no longer fits `have` bytes - then
 * plan returns twice the block's size for the caller to allocate, else `have`.  send() packs every maximal run of such sections
 * into staging and hands the caller one copy (dst_offset, src, bytes) per run, from the first section's offset to the next
 * current section's offset or the block end; then the single elements of sections that did not go up anyway, from the host array
 * itself.  It points the device view at `base`, adds the bytes to the caller's counter and returns them.  An empty section takes
 * no room and sends nothing.
 *
 * A section may be granted a capacity, in elements (grant(), section_of()): room behind its elements, so that an array that is
 * only appended to keeps its offset and those of the sections behind it.  Such a section takes max(size, capacity) elements of
 * room, empty or not.  When it has grown since the last send, inside its room, without a mark and without moving, only the new
 * tail goes up, from the host array itself: the caller appended and changed nothing below.  grant(section, need) leaves a capacity
 * that holds `need` elements alone and else sets it to twice `need`, which moves the sections behind (they go up once) and
 * returns true.  A block without a granted section lays out, plans and sends exactly as described above. */
#ifndef DRFE_RESIDENT_BLOCK_H
#define DRFE_RESIDENT_BLOCK_H

#include "stage_layout.h"

#include <stdint.h>
#include <type_traits>
#include <utility>
#include <vector>

class ResidentBlock {
public:
    ResidentBlock() = default;
    ResidentBlock(const ResidentBlock&) = delete;
    ResidentBlock& operator=(const ResidentBlock&) = delete;

    /* the next section; P is T* or const T*, as the views declare the field */
    template <class T, class P>
    int bind(std::vector<T>& v, P* dev, P* host = nullptr)
    {
        static_assert(std::is_same<P, T*>::value || std::is_same<P, const T*>::value, "a view's field points at the array's elements");
        static_assert(16 % alignof(T) == 0, "element type over-aligned for a section");
        Bound b;
        b.vec = &v;
        b.dev = dev;
        b.host = host;
        b.elem = sizeof(T);
        b.span = [](void* vec, size_t* n) {
            std::vector<T>* w = static_cast<std::vector<T>*>(vec);
            *n = w->size();
            return reinterpret_cast<char*>(w->data());
        };
        b.point = [](void* field, char* p) { *static_cast<P*>(field) = reinterpret_cast<P>(p); };
        s_.push_back(b);
        return (int)s_.size() - 1;
    }

    /* last < 0: to the end of the block */
    void stale(int first, int last = -1)
    {
        for (size_t i = (size_t)first; i < s_.size() && (last < 0 || i <= (size_t)last); i++) s_[i].marked = true;
    }
    void stale_all()
    {
        stale(0);
        elems_.clear();
    }
    void stale_at(int section, size_t index) { elems_.emplace_back(section, index); }

    /* the section bound to this vector, or -1 */
    int section_of(const void* vec) const
    {
        for (size_t i = 0; i < s_.size(); i++)
            if (s_[i].vec == vec) return (int)i;
        return -1;
    }
    /* room for `need` elements in the section: true when its capacity had to be set anew, to twice `need` */
    bool grant(int section, size_t need)
    {
        Bound& b = s_[(size_t)section];
        if (need * b.elem <= b.cap) return false;
        b.cap = 2 * need * b.elem;
        return true;
    }
    /* a device call appended to the section itself, inside its room, what the host array now holds too */
    void took(int section)
    {
        Bound& b = s_[(size_t)section];
        size_t n;
        b.span(b.vec, &n);
        if (!b.marked && b.off == b.heldOff && n * b.elem <= (b.cap > b.heldBytes ? b.cap : b.heldBytes)) b.heldBytes = n * b.elem;
    }
    size_t capacity(int section) const { return s_[(size_t)section].cap / s_[(size_t)section].elem; }
    void assume_current()
    {
        for (Bound& b : s_) b.marked = false;
        elems_.clear();
    }

    size_t plan(size_t have)
    {
        StageLayout<16> L;
        for (Bound& b : s_) {
            size_t n;
            b.span(b.vec, &n);
            b.bytes = n * b.elem;
            b.off = L.add<char>(b.bytes > b.cap ? b.bytes : b.cap).off;
        }
        bytes_ = L.bytes();
        if (bytes_ > have) stale_all();
        staged_ = 0;
        for (size_t i = 0; i < s_.size(); i++) {
            Bound& b = s_[i];
            /* appended to inside its room: the tail alone */
            b.tail = !b.marked && b.off == b.heldOff && b.bytes > b.heldBytes && b.bytes <= b.cap;
            b.up = !b.tail && (b.marked || b.off != b.heldOff || b.bytes != b.heldBytes);
            if (b.up) staged_ += end(i) - b.off;
        }
        return bytes_ > have ? 2 * bytes_ : have;
    }
    size_t bytes() const { return bytes_; }    /* of the block as planned */
    size_t staged() const { return staged_; }  /* of staging that send() will fill */

    template <class Copy>
    size_t send(char* base, char* stage, Copy&& copy, int64_t* counter)
    {
        size_t sent = 0;
        for (size_t i = 0; i < s_.size();) {
            if (!s_[i].up) {
                i++;
                continue;
            }
            const size_t from = s_[i].off;
            for (; i < s_.size() && s_[i].up; i++) {
                size_t n;
                const char* src = s_[i].span(s_[i].vec, &n);
                if (s_[i].bytes) memcpy(stage + sent + (s_[i].off - from), src, s_[i].bytes);
            }
            const size_t run = end(i - 1) - from;
            if (run) copy(from, stage + sent, run);
            sent += run;
        }
        for (const std::pair<int, size_t>& e : elems_) {
            const Bound& b = s_[(size_t)e.first];
            size_t n;
            const char* src = b.span(b.vec, &n);
            if (b.up || e.second >= n) continue;
            copy(b.off + e.second * b.elem, src + e.second * b.elem, b.elem);
            sent += b.elem;
        }
        for (const Bound& b : s_) {
            if (!b.tail) continue;
            size_t n;
            const char* src = b.span(b.vec, &n);
            copy(b.off + b.heldBytes, src + b.heldBytes, b.bytes - b.heldBytes);
            sent += b.bytes - b.heldBytes;
        }
        for (Bound& b : s_) {
            b.tail = false;
            b.heldOff = b.off;
            b.heldBytes = b.bytes;
            b.up = false;
            b.point(b.dev, base + b.off);
        }
        assume_current();
        if (counter) *counter += (int64_t)sent;
        return sent;
    }

    /* the host view's fields onto the arrays where they are now: a vector's data() moves */
    void point_host()
    {
        size_t n;
        for (Bound& b : s_)
            if (b.host) b.point(b.host, b.span(b.vec, &n));
    }

private:
    struct Bound {
        void *vec, *dev, *host;
        size_t elem;
        char* (*span)(void* vec, size_t* n);
        void (*point)(void* field, char* p);
        size_t off = 0, bytes = 0;                         /* as planned */
        size_t heldOff = (size_t)-1, heldBytes = 0;        /* what the device copy holds */
        size_t cap = 0;                                    /* granted room in bytes, 0 = none */
        bool marked = true, up = false, tail = false;
    };
    size_t end(size_t i) const { return i + 1 < s_.size() ? s_[i + 1].off : bytes_; }

    std::vector<Bound> s_;
    std::vector<std::pair<int, size_t>> elems_;
    size_t bytes_ = 0, staged_ = 0;
};

#endif
