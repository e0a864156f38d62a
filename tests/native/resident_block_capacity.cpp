/* resident_block_capacity.cpp — the granted capacities of ResidentBlock (dr_slam_amd/csrc/resident_block.h) against a fake device,
 * a std::vector<char>: one block of three sections (uint8_t, int32_t, int32_t).  Without a grant the layout is the packed one;
 * a granted section keeps its offset while it grows inside its room and sends only its new tail; one element beyond the room lays
 * the block out anew, once; an empty section with a grant holds its room; a section a device call appended to itself is taken as
 * current.  After every step each section of the fake device must equal the host array at the offset the view points to, and the
 * copies and bytes must be the figures written here, which follow by hand from the sizes and the 16-byte alignment.  No HIP call.
 * tests/test_resident_block_capacity_cpu.py builds and runs it. */
#include "../../dr_slam_amd/csrc/resident_block.h"

#include <stdio.h>

namespace {

struct View {
    const uint8_t* a;
    const int32_t* b;
    int32_t* c;
};

struct Rig {
    std::vector<uint8_t> a;
    std::vector<int32_t> b, c;
    View dv;
    ResidentBlock B;
    int sa, sb, sc;
    std::vector<char> dev, stage;
    int64_t counter = 0;
    int copies = 0, failed = 0, steps = 0, salt = 0;
    size_t firstDst = 0;

    Rig()
    {
        dv = View{(const uint8_t*)1, (const int32_t*)1, (int32_t*)1};
        sa = B.bind(a, &dv.a);
        sb = B.bind(b, &dv.b);
        sc = B.bind(c, &dv.c);
    }

    void check(bool ok, const char* step, const char* what)
    {
        if (ok) return;
        printf("FAILED %s: %s\n", step, what);
        failed++;
    }

    /* n more elements behind the stored ones, which stay as they are */
    void append(std::vector<int32_t>& v, int n)
    {
        for (int i = 0; i < n; i++) v.push_back(1000 * ++salt + (int32_t)v.size());
    }

    /* one sync; offsets of the three sections, the first copy's destination, copies, bytes and the device size afterwards */
    void sync(const char* step, const size_t (&off)[3], size_t dst, int wantCopies, int64_t wantBytes, size_t wantCapacity)
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
        check((const char*)dv.a == base + off[0] && (const char*)dv.b == base + off[1] && (const char*)dv.c == base + off[2], step,
              "the device view's offsets");
        check(!memcmp(dv.a, a.data(), a.size()) && !memcmp(dv.b, b.data(), 4 * b.size()) && !memcmp(dv.c, c.data(), 4 * c.size()), step,
              "the device copy's contents");
    }
};

}  // namespace

int main()
{
    Rig R;
    /* 5 x 1, 7 x 4, 10 x 4 bytes: extents 16, 32, 48.  No capacity: the packed layout, one copy of the whole block */
    R.a.assign(5, 9);
    R.append(R.b, 7);
    R.append(R.c, 10);
    R.sync("no capacity", {0, 16, 48}, 0, 1, 96, 192);
    R.check(R.B.capacity(R.sb) == 0 && R.B.section_of(&R.b) == R.sb && R.B.section_of(&R.dev) == -1, "no capacity", "capacity / section_of");
    R.sync("nothing changed", {0, 16, 48}, 0, 0, 0, 192);
    /* b is granted room for 10: twice that, 20 x 4 = 80 bytes, so c moves from 48 to 96 and goes up (extent 48, the first copy);
     * b stays at 16 and sends its 3 new elements, 12 bytes at 16 + 28.  The block ends at 144 */
    R.check(R.B.grant(R.sb, 10) && R.B.capacity(R.sb) == 20, "grant", "a first grant sets twice the need");
    R.append(R.b, 3);
    R.sync("granted and appended", {0, 16, 96}, 96, 2, 60, 192);
    /* growth inside the room: the tail alone, 5 x 4 bytes at 16 + 40 */
    R.check(!R.B.grant(R.sb, 15), "inside", "no new grant inside the room");
    R.append(R.b, 5);
    R.sync("growth inside the capacity", {0, 16, 96}, 56, 1, 20, 192);
    /* to the last element of the room: 5 x 4 bytes at 16 + 60 */
    R.check(!R.B.grant(R.sb, 20), "exact", "the room holds exactly 20");
    R.append(R.b, 5);
    R.sync("filling the capacity", {0, 16, 96}, 76, 1, 20, 192);
    /* a marked section goes up whole with its room, tail or not: 80 bytes from 16 */
    R.b[0] = -5;
    R.B.stale(R.sb, R.sb);
    R.sync("marked inside the capacity", {0, 16, 96}, 16, 1, 80, 192);
    /* one element beyond: room for 42, 168 bytes, c at 16 + 168 = 184 -> 192, the block ends at 240 > 192: a new allocation of
     * 480 and the whole block in one copy.  Then nothing more */
    R.check(R.B.grant(R.sb, 21) && R.B.capacity(R.sb) == 42, "beyond", "one beyond the room doubles it");
    R.append(R.b, 1);
    R.sync("one element beyond the capacity", {0, 16, 192}, 0, 1, 240, 480);
    R.sync("relaid out once", {0, 16, 192}, 0, 0, 0, 480);
    /* a device call appends two elements to b inside the room and the host commits the same values: nothing travels */
    R.append(R.b, 2);
    memcpy(R.dev.data() + 16 + 4 * 21, R.b.data() + 21, 8);
    R.B.took(R.sb);
    R.sync("appended on the device", {0, 16, 192}, 0, 0, 0, 480);
    /* c emptied and granted room for 4 (8 x 4 = 32 bytes): it keeps that room at 192, the block ends at 224; its run goes up (32
     * bytes of room, no element).  Then two elements: 8 bytes at 192 */
    R.c.clear();
    R.check(R.B.grant(R.sc, 4) && R.B.capacity(R.sc) == 8, "empty", "a grant on an empty section");
    R.sync("an empty section with a capacity", {0, 16, 192}, 192, 1, 32, 480);
    R.append(R.c, 2);
    R.sync("its first elements", {0, 16, 192}, 192, 1, 8, 480);
    /* a emptied, no capacity: it takes no room, b moves to 0 and c to 176: everything goes up in one copy of 176 + 32 bytes */
    R.a.clear();
    R.sync("an empty section without a capacity", {0, 0, 176}, 0, 1, 208, 480);
    printf("steps %d failed %d\n", R.steps, R.failed);
    return R.failed ? 1 : 0;
}
