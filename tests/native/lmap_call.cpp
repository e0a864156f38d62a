/* lmap_call.cpp — the two parts of dr_slam_amd/csrc/lmap_call.h that are free of HIP, against a fake device, a std::vector<char>.
 * LmapFetch: sections of element sizes 1, 4, 8 and 12 at counts 0, 1, 3, 4, 5 and 300 in mixed order, all empty, a single trailing
 * empty section, and one object run again at smaller counts and at the counts it was sized for.  After every run each section of
 * the host block must equal the fake device at its source, and the copies, their bytes, the block's bytes and the offsets must be
 * the figures written here, which follow by hand from the counts, the element sizes and the 16-byte alignment.
 * LmapWrites: against a ResidentBlock bound to two small vectors; what the next plan stages says whether the blocks were left to be
 * sent again.  No HIP call: the copy is a memcpy.  tests/test_lmap_call_cpu.py builds and runs it. */
#include "../../dr_slam_amd/csrc/lmap_call.h"

#include <stdio.h>

namespace {

struct F3 {
    float v[3];
};
static_assert(sizeof(F3) == 12, "three floats");

int steps = 0, failed = 0;

void check(bool ok, const char* step, const char* what)
{
    if (ok) return;
    printf("FAILED %s: %s\n", step, what);
    failed++;
}

/* the fake device: every byte differs from its neighbours and from the host block's fill */
struct Device {
    std::vector<char> mem;
    Device() : mem(8192)
    {
        for (size_t i = 0; i < mem.size(); i++) mem[i] = (char)(1 + (i * 7 + i / 251) % 250);
    }
    template <class T>
    const T* at(size_t byte) const { return reinterpret_cast<const T*>(mem.data() + byte); }
};

struct Run {
    std::vector<char> host;
    int copies = 0;
    size_t bytes = 0;
    bool inside = true, aligned = true;

    /* one run of the fetch into a block of `room` bytes */
    void go(LmapFetch& f, const Device& D, size_t room)
    {
        host.assign(room + 16, (char)0);
        copies = 0;
        bytes = 0;
        inside = aligned = true;
        char* base = host.data();
        f.run(base, [&](void* dst, const void* src, size_t n) {
            copies++;
            bytes += n;
            const size_t off = (size_t)((char*)dst - base);
            if (off % 16) aligned = false;
            if (off + n > room || (const char*)src < D.mem.data() || (const char*)src + n > D.mem.data() + D.mem.size()) {
                inside = false;
                return;
            }
            memcpy(dst, src, n);
        });
    }
};

/* a section holds what the fake device holds at src, at a 16-aligned offset of the block */
template <class T>
bool holds(const LmapFetch& f, Fetched<T> s, const Run& R, const T* src, size_t n)
{
    const size_t off = (size_t)((const char*)f.at(s) - R.host.data());
    return f.n(s) == n && off % 16 == 0 && (!n || !memcmp(f.at(s), src, n * sizeof(T)));
}

void verdict(const Run& R, const char* step, int wantCopies, size_t wantBytes)
{
    check(R.copies == wantCopies, step, "copies");
    check(R.bytes == wantBytes, step, "bytes copied");
    check(R.inside, step, "a copy outside the host block or the device");
    check(R.aligned, step, "a copy to an offset that is no multiple of 16");
}

void fetch_mixed(const Device& D)
{
    const char* step = "mixed sizes and counts";
    steps++;
    /* sources at odd places of the device; extents 304, 0, 16, 16, 48, 16, 16, 0, 3600, 48: the block is 4064 bytes */
    LmapFetch f;
    const auto a = f.add(D.at<uint8_t>(3), 300);      /* 300 bytes at 0 */
    const auto b = f.add(D.at<int32_t>(400), 0);      /* nothing at 304 */
    const auto c = f.add(D.at<double>(408), 1);       /* 8 at 304 */
    const auto d = f.add(D.at<int32_t>(420), 3);      /* 12 at 320 */
    const auto e = f.add(D.at<F3>(440), 4);           /* 48 at 336 */
    const auto g = f.add(D.at<uint8_t>(501), 5);      /* 5 at 384 */
    const auto h = f.add(D.at<int32_t>(512), 4);      /* 16 at 400 */
    const auto i = f.add(D.at<double>(600), 0);       /* nothing at 416 */
    const auto j = f.add(D.at<F3>(1000), 300);        /* 3600 at 416 */
    const auto k = f.add(D.at<double>(4800), 5);      /* 40 at 4016 */
    check(f.bytes() == 4064, step, "the block's bytes");
    Run R;
    R.go(f, D, f.bytes());
    verdict(R, step, 8, 300 + 8 + 12 + 48 + 5 + 16 + 3600 + 40);
    check(holds(f, a, R, D.at<uint8_t>(3), 300) && holds(f, b, R, D.at<int32_t>(400), 0) && holds(f, c, R, D.at<double>(408), 1) &&
              holds(f, d, R, D.at<int32_t>(420), 3) && holds(f, e, R, D.at<F3>(440), 4) && holds(f, g, R, D.at<uint8_t>(501), 5) &&
              holds(f, h, R, D.at<int32_t>(512), 4) && holds(f, i, R, D.at<double>(600), 0) && holds(f, j, R, D.at<F3>(1000), 300) &&
              holds(f, k, R, D.at<double>(4800), 5), step, "a section's contents");
    check((const char*)f.at(c) == R.host.data() + 304 && (const char*)f.at(e) == R.host.data() + 336 &&
              (const char*)f.at(j) == R.host.data() + 416 && (const char*)f.at(k) == R.host.data() + 4016, step, "the offsets");
    /* get() takes a section's elements out, and nothing of an empty one */
    int32_t out[4] = {-1, -1, -1, -1};
    f.get(d, out);
    f.get(b, out + 3);
    check(!memcmp(out, D.at<int32_t>(420), 12) && out[3] == -1, step, "get");
}

void fetch_empty(const Device& D)
{
    steps++;
    LmapFetch f;
    const auto a = f.add(D.at<int32_t>(16), 0);
    const auto b = f.add(D.at<F3>(32), 0);
    const auto c = f.add(D.at<uint8_t>(48), 0);
    Run R;
    R.go(f, D, 0);
    check(f.bytes() == 0, "all empty", "the block's bytes");
    verdict(R, "all empty", 0, 0);
    check(f.n(a) == 0 && f.n(b) == 0 && f.n(c) == 0, "all empty", "the counts");

    steps++;
    /* 5 x 4 = 20 bytes, extent 32; 3 x 8 = 24 at 32, extent 32; nothing at 64 */
    LmapFetch t;
    const auto p = t.add(D.at<int32_t>(100), 5);
    const auto q = t.add(D.at<double>(200), 3);
    const auto r = t.add(D.at<F3>(300), 0);
    R.go(t, D, t.bytes());
    check(t.bytes() == 64, "a trailing empty section", "the block's bytes");
    verdict(R, "a trailing empty section", 2, 20 + 24);
    check(holds(t, p, R, D.at<int32_t>(100), 5) && holds(t, q, R, D.at<double>(200), 3) && holds(t, r, R, D.at<F3>(300), 0),
          "a trailing empty section", "a section's contents");
}

/* the chunked use: sized once for the fullest chunk, then run at each chunk's counts without growing */
void fetch_again(const Device& D)
{
    /* rooms 1 x 4, 5 x 4, 5 x 12, 5 x 1: extents 16, 32, 64, 16: 128 bytes */
    LmapFetch f;
    const auto tot = f.add(D.at<int32_t>(2000), 1);
    const auto item = f.add(D.at<int32_t>(2100), 5);
    const auto world = f.add(D.at<F3>(2200), 5);
    const auto kind = f.add(D.at<uint8_t>(2300), 5);
    const size_t room = f.bytes();
    check(room == 128, "sized for the fullest chunk", "the block's bytes");
    Run R;

    steps++;
    const char* step = "a smaller chunk";
    f.set(tot, D.at<int32_t>(2004), 1);               /* the one word moves, as a chunk's total does */
    f.set(3, item, world, kind);
    R.go(f, D, room);
    verdict(R, step, 4, 4 + 12 + 36 + 3);
    check(f.bytes() == room, step, "the block's bytes moved");
    check(holds(f, tot, R, D.at<int32_t>(2004), 1) && holds(f, item, R, D.at<int32_t>(2100), 3) && holds(f, world, R, D.at<F3>(2200), 3) &&
              holds(f, kind, R, D.at<uint8_t>(2300), 3), step, "a section's contents");
    check((const char*)f.at(item) == R.host.data() + 16 && (const char*)f.at(world) == R.host.data() + 48 &&
              (const char*)f.at(kind) == R.host.data() + 112, step, "the offsets");
    /* the elements past a chunk's count are not touched */
    check(R.host[16 + 12] == 0 && R.host[48 + 36] == 0 && R.host[112 + 3] == 0, step, "a copy past the count");

    steps++;
    step = "a chunk with nothing but its total";
    f.set(0, item, world, kind);
    R.go(f, D, room);
    verdict(R, step, 1, 4);
    check(holds(f, tot, R, D.at<int32_t>(2004), 1) && f.n(item) == 0 && f.n(world) == 0 && f.n(kind) == 0, step, "a section's contents");

    steps++;
    step = "the fullest chunk";
    f.set(tot, D.at<int32_t>(2000), 1);
    f.set(5, item, world, kind);
    R.go(f, D, room);
    verdict(R, step, 4, 4 + 20 + 60 + 5);
    check(f.bytes() == room, step, "the block's bytes moved");
    check(holds(f, tot, R, D.at<int32_t>(2000), 1) && holds(f, item, R, D.at<int32_t>(2100), 5) && holds(f, world, R, D.at<F3>(2200), 5) &&
              holds(f, kind, R, D.at<uint8_t>(2300), 5), step, "a section's contents");
}

/* a ResidentBlock of two arrays, 3 x 4 and 5 x 1 bytes: extents 16 and 16, 32 bytes in all */
struct Block {
    std::vector<int32_t> a{1, 2, 3};
    std::vector<uint8_t> b{4, 5, 6, 7, 8};
    const int32_t* da = nullptr;
    const uint8_t* db = nullptr;
    ResidentBlock B;
    std::vector<char> dev, stage;

    Block() : dev(64)
    {
        B.bind(a, &da);
        B.bind(b, &db);
        check(sync() == 32, "the guard's block", "its first sync");
    }
    /* the bytes the next upload sends */
    size_t sync()
    {
        B.plan(dev.size());
        stage.assign(B.staged(), (char)0);
        return B.send(dev.data(), stage.data(), [&](size_t o, const void* src, size_t n) { memcpy(dev.data() + o, src, n); }, nullptr);
    }
};

int call_that_writes(Block& one, Block& two, bool arm, bool finish)
{
    if (!arm) return 1;                /* refused before the first writing launch */
    LmapWrites writes(one.B, &two.B);
    if (!finish) return 2;             /* a failure after it */
    writes.done();
    return 0;
}

void guard()
{
    Block one, two;
    steps++;
    check(call_that_writes(one, two, true, true) == 0 && one.sync() == 0 && two.sync() == 0, "armed then done", "a block was sent again");
    steps++;
    check(call_that_writes(one, two, true, false) == 2 && one.sync() == 32 && two.sync() == 32, "armed then dropped", "a block was not sent whole");
    steps++;
    check(call_that_writes(one, two, false, false) == 1 && one.sync() == 0 && two.sync() == 0, "not armed", "a block was sent again");
    steps++;
    {
        LmapWrites alone(one.B);
    }
    check(one.sync() == 32 && two.sync() == 0, "one block named", "the other block moved, or the named one did not");
}

}  // namespace

int main()
{
    const Device D;
    fetch_mixed(D);
    fetch_empty(D);
    fetch_again(D);
    guard();
    printf("steps %d failed %d\n", steps, failed);
    return failed ? 1 : 0;
}
