/* resident_block.cpp — ResidentBlock (dr_slam_amd/csrc/resident_block.h) against a fake device, a std::vector<char>: one block of
 * five sections of mixed element types through every kind of edit.  After every step each section of the fake device must equal
 * the host array at the offset the view points to, and the copies and bytes must be the figures written here, which follow by hand
 * from the sizes and the 16-byte alignment.  No HIP call: the copy is a memcpy.  tests/test_resident_block_cpu.py builds and runs it. */
#include "../../dr_slam_amd/csrc/resident_block.h"

#include <stdio.h>

namespace {

struct View {
    const uint8_t* a;
    const int32_t* b;
    float* c;
    const double* d;
    int32_t* e;
};

struct Rig {
    std::vector<uint8_t> a;
    std::vector<int32_t> b;
    std::vector<float> c;
    std::vector<double> d;
    std::vector<int32_t> e;
    View dv, hv;
    ResidentBlock B;
    std::vector<char> dev, stage;
    int64_t counter = 0;
    int copies = 0, failed = 0, steps = 0;
    size_t firstDst = 0;

    Rig()
    {
        dv = hv = View{(const uint8_t*)1, (const int32_t*)1, (float*)1, (const double*)1, (int32_t*)1};
        B.bind(a, &dv.a, &hv.a);
        B.bind(b, &dv.b, &hv.b);
        B.bind(c, &dv.c, &hv.c);
        B.bind(d, &dv.d);
        B.bind(e, &dv.e, &hv.e);
    }

    /* new values everywhere, so that a section that wrongly stayed behind shows */
    void scribble(int salt)
    {
        for (size_t i = 0; i < a.size(); i++) a[i] = (uint8_t)(salt + 3 * i);
        for (size_t i = 0; i < b.size(); i++) b[i] = salt * 1000 + (int32_t)i;
        for (size_t i = 0; i < c.size(); i++) c[i] = (float)salt + 0.25f * (float)i;
        for (size_t i = 0; i < d.size(); i++) d[i] = (double)salt * 1e9 + (double)i;
        for (size_t i = 0; i < e.size(); i++) e[i] = -salt * 1000 - (int32_t)i;
    }

    void check(bool ok, const char* step, const char* what)
    {
        if (ok) return;
        printf("FAILED %s: %s\n", step, what);
        failed++;
    }

    /* one sync; offsets of the five sections, the first copy's destination, copies, bytes and the device size afterwards */
    void sync(const char* step, const size_t (&off)[5], size_t dst, int wantCopies, int64_t wantBytes, size_t wantCapacity)
    {
        steps++;
        const size_t want = B.plan(dev.size());
        if (want != dev.size()) dev.assign(want, (char)0xEE);      /* like a new allocation: the old contents are gone */
        stage.assign(B.staged(), (char)0x55);
        copies = 0;
        const int64_t before = counter;
        char* base = dev.data();
        const size_t sent = B.send(base, stage.data(), [&](size_t o, const void* src, size_t n) {
            if (!copies++) firstDst = o;
            check(o + n <= dev.size(), step, "a copy past the device block");
            if (o + n <= dev.size()) memcpy(base + o, src, n);
        }, &counter);
        check(copies == wantCopies, step, "copies");
        check(counter - before == wantBytes && (int64_t)sent == wantBytes, step, "bytes");
        check(!wantCopies || firstDst == dst, step, "where the first copy starts");
        check(dev.size() == wantCapacity, step, "capacity");
        check((const char*)dv.a == base + off[0] && (const char*)dv.b == base + off[1] && (const char*)dv.c == base + off[2] &&
                  (const char*)dv.d == base + off[3] && (const char*)dv.e == base + off[4], step, "the device view's offsets");
        check(!memcmp(dv.a, a.data(), a.size()) && !memcmp(dv.b, b.data(), 4 * b.size()) && !memcmp(dv.c, c.data(), 4 * c.size()) &&
                  !memcmp(dv.d, d.data(), 8 * d.size()) && !memcmp(dv.e, e.data(), 4 * e.size()), step, "the device copy's contents");
        B.point_host();
        check(hv.a == a.data() && hv.b == b.data() && hv.c == c.data() && hv.e == e.data(), step, "the host view");
    }
};

}  // namespace

int main()
{
    Rig R;
    /* 5 x 1, 7 x 4, 3 x 4, 4 x 8, 10 x 4 bytes: extents 16, 32, 16, 32, 48 */
    R.a.resize(5);
    R.b.resize(7);
    R.c.resize(3);
    R.d.resize(4);
    R.e.resize(10);
    R.scribble(1);
    R.sync("first sync", {0, 16, 48, 64, 96}, 0, 1, 144, 288);
    R.sync("nothing marked", {0, 16, 48, 64, 96}, 0, 0, 0, 288);
    R.a[0] ^= 0x80;
    R.b[6] = 77;
    R.B.stale(0, 1);
    R.sync("first two sections", {0, 16, 48, 64, 96}, 0, 1, 48, 288);
    /* the last array shrinks to 6 x 4 = 24 bytes, extent 32: the block ends at 128 */
    R.e.resize(6);
    R.d[1] = -1.0;
    R.e[5] = 5;
    R.B.stale(3, 4);
    R.sync("tail after a shrink", {0, 16, 48, 64, 96}, 64, 1, 64, 288);
    R.a[4] = 9;
    R.e[0] = 1;
    R.B.stale(0, 0);
    R.B.stale(4);
    R.sync("prefix and tail", {0, 16, 48, 64, 96}, 0, 2, 16 + 32, 288);
    /* the middle array grows to 9 x 4 = 36 bytes, extent 48: d and e move by 32, the block ends at 160 */
    R.c.assign(9, 2.5f);
    R.e[1] = 2;
    R.B.stale(4);
    R.sync("a middle array resized", {0, 16, 48, 96, 128}, 48, 1, 160 - 48, 288);
    /* b grows to 80 x 4 = 320 bytes: the block is 16 + 320 + 48 + 32 + 32 = 448 > 288, allocated at 896 */
    R.b.resize(80);
    R.scribble(2);
    R.sync("growth past capacity", {0, 16, 336, 384, 416}, 0, 1, 448, 896);
    /* c empties: d and e move up by 48; nothing is marked */
    R.c.clear();
    R.sync("a middle section of zero elements", {0, 16, 336, 336, 368}, 336, 1, 64, 896);
    R.scribble(3);
    R.B.stale_all();
    R.B.assume_current();
    R.steps++;
    R.B.plan(R.dev.size());
    R.check(R.B.staged() == 0, "assume_current after stale_all", "staged bytes");
    R.B.stale_all();
    R.sync("everything again", {0, 16, 336, 336, 368}, 0, 1, 400, 896);
    /* single elements: 4 bytes each from the host array; the one in a section that goes up anyway is dropped */
    R.e[3] = 33;
    R.b[2] = 22;
    R.B.stale_at(4, 3);
    R.B.stale_at(1, 2);
    R.B.stale(1, 1);
    R.sync("single elements", {0, 16, 336, 336, 368}, 16, 2, 320 + 4, 896);

    /* a block whose arrays are all empty: nothing to allocate, no copy, the views point at the base */
    Rig E;
    char nothing = 0;
    E.steps++;
    const size_t want = E.B.plan(0);
    int copies = 0;
    const size_t sent = E.B.send(&nothing, nullptr, [&](size_t, const void*, size_t) { copies++; }, &E.counter);
    E.check(want == 0 && E.B.bytes() == 0 && E.B.staged() == 0 && sent == 0 && copies == 0 && E.counter == 0, "an empty block", "it sent something");
    E.check((const char*)E.dv.a == &nothing && (const char*)E.dv.c == &nothing && (const char*)E.dv.e == &nothing, "an empty block", "the views");

    printf("steps %d failed %d\n", R.steps + E.steps, R.failed + E.failed);
    return R.failed + E.failed ? 1 : 0;
}
