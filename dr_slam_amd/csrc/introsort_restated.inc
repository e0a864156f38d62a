/* introsort_restated.inc — the partition phase of introsort_restated.h, compiled once per (record type, order, instruction set).
 * The including file defines
 *   ISR_NS      namespace of this instance
 *   ISR_REC     record type (uint32_t / uint64_t)
 *   ISR_SHIFT   the sort key of a record v is v >> ISR_SHIFT (fits 31 bits: the signed vector compares are exact)
 *   ISR_DESC    1: larger keys first (LSD's compare_norm), 0: smaller keys first (VoxelGrid's cloud_point_index_idx)
 *   ISR_TARGET  function attribute, ISR_AVX2 0 / 1
 * Every function carries the target attribute so that the mask routines inline into the partition loop. */
namespace ISR_NS {

typedef ISR_REC rec_t;
static inline uint32_t key_of(rec_t v) { return (uint32_t)(v >> ISR_SHIFT); }
/* the comparator std::sort is called with: a goes before b */
struct Before {
    bool operator()(rec_t a, rec_t b) const { return ISR_DESC ? key_of(a) > key_of(b) : key_of(a) < key_of(b); }
};

/* bit t set iff key(a[t]) > pk (kGreater) resp. pk > key(a[t]) */
#if ISR_AVX2
ISR_TARGET static inline uint64_t mask_gt(const rec_t* a, uint32_t pk, bool kGreater)
{
    uint64_t m = 0;
    if (sizeof(rec_t) == 4) {
        const __m256i ref = _mm256_set1_epi32((int)pk);
        for (int t = 0; t < 64; t += 8) {
            const __m256i k = _mm256_srli_epi32(_mm256_loadu_si256((const __m256i*)(a + t)), ISR_SHIFT & 31);
            const __m256i c = kGreater ? _mm256_cmpgt_epi32(k, ref) : _mm256_cmpgt_epi32(ref, k);
            m |= (uint64_t)(uint32_t)_mm256_movemask_ps(_mm256_castsi256_ps(c)) << t;
        }
    } else {
        const __m256i ref = _mm256_set1_epi64x((long long)pk);
        for (int t = 0; t < 64; t += 4) {
            const __m256i k = _mm256_srli_epi64(_mm256_loadu_si256((const __m256i*)(a + t)), ISR_SHIFT);
            const __m256i c = kGreater ? _mm256_cmpgt_epi64(k, ref) : _mm256_cmpgt_epi64(ref, k);
            m |= (uint64_t)(uint32_t)_mm256_movemask_pd(_mm256_castsi256_pd(c)) << t;
        }
    }
    return m;
}
#else
static inline uint64_t mask_gt(const rec_t* a, uint32_t pk, bool kGreater)
{
    uint64_t m = 0;
    if (kGreater) for (int t = 0; t < 64; t++) m |= (uint64_t)(key_of(a[t]) > pk) << t;
    else for (int t = 0; t < 64; t++) m |= (uint64_t)(pk > key_of(a[t])) << t;
    return m;
}
#endif
/* the scan from the left passes records that go before the pivot and stops at the others; the scan from the right passes records
 * the pivot goes before */
ISR_TARGET static inline uint64_t mask_left(const rec_t* a, uint32_t pk) { return ~mask_gt(a, pk, ISR_DESC != 0); }
ISR_TARGET static inline uint64_t mask_right(const rec_t* a, uint32_t pk) { return ~mask_gt(a, pk, ISR_DESC == 0); }
static inline bool stops_left(rec_t v, uint32_t pk) { return ISR_DESC ? !(key_of(v) > pk) : !(key_of(v) < pk); }
static inline bool stops_right(rec_t v, uint32_t pk) { return ISR_DESC ? !(pk > key_of(v)) : !(pk < key_of(v)); }

/* std::__unguarded_partition(a + lo, a + hi, pivot) for a pivot of key pk: returns the cut */
ISR_TARGET static inline size_t hoare_cut(rec_t* a, size_t lo, size_t hi, uint32_t pk)
{
    size_t i = lo, j = hi;                        /* [i, j): not yet scanned */
    if (hi - lo > 256) {
        /* two blocks of 64 that cannot meet: every left stopper lies left of every right stopper, all pairs swap */
        uint64_t mL = 0, mR = 0;
        size_t baseL = 0, baseR = 0;
        while (j - i >= 128) {
            if (!mL) { baseL = i; mL = mask_left(a + i, pk); i += 64; }
            if (!mR) { j -= 64; baseR = j; mR = mask_right(a + j, pk); }
            while (mL && mR) {
                const int l = __builtin_ctzll(mL), r = 63 - __builtin_clzll(mR);
                std::swap(a[baseL + l], a[baseR + r]);
                mL &= mL - 1;
                mR ^= 1ull << r;
            }
        }
        /* back to the sequential algorithm's state: its left pointer rests on the first unconsumed left stopper (everything
         * after it in the block is untouched), its right pointer one past the first unconsumed right stopper */
        if (mL) i = baseL + __builtin_ctzll(mL);
        if (mR) j = baseR + (63 - __builtin_clzll(mR)) + 1;
    }
    /* the rest, <= 256 records: both stopper sets of the whole range, then pair them off.  Everything right of j stops a left
     * scan and everything left of i stops a right scan, so "no stopper left" reads j resp. "stop" */
    const size_t n = j - i;
    const int W = (int)((n + 63) >> 6);
    uint64_t ML[4], MR[4];
    for (int w = 0; w < W; w++) {
        const size_t off = i + ((size_t)w << 6);
        if (off + 64 <= j) { ML[w] = mask_left(a + off, pk); MR[w] = mask_right(a + off, pk); }
        else {
            uint64_t l = 0, r = 0;
            for (size_t t = 0; off + t < j; t++) {
                l |= (uint64_t)stops_left(a[off + t], pk) << t;
                r |= (uint64_t)stops_right(a[off + t], pk) << t;
            }
            ML[w] = l; MR[w] = r;
        }
    }
    int lw = 0, rw = W - 1;
    size_t prevR = j;
    for (;;) {
        while (lw < W && !ML[lw]) lw++;
        while (rw >= 0 && !MR[rw]) rw--;
        const size_t l = lw < W ? i + ((size_t)lw << 6) + (size_t)__builtin_ctzll(ML[lw]) : j;
        if (rw < 0) return std::min(l, prevR);
        const int rb = 63 - __builtin_clzll(MR[rw]);
        const size_t r = i + ((size_t)rw << 6) + (size_t)rb;
        if (!(l < r)) return std::min(l, prevR);
        std::swap(a[l], a[r]);
        ML[lw] &= ML[lw] - 1;
        MR[rw] ^= 1ull << rb;
        prevR = r;
    }
}

/* std::__move_median_to_first(result, x, y, z) */
static inline void median_to_first(rec_t* a, size_t result, size_t x, size_t y, size_t z)
{
    const Before before;
    if (before(a[x], a[y])) {
        if (before(a[y], a[z])) std::swap(a[result], a[y]);
        else if (before(a[x], a[z])) std::swap(a[result], a[z]);
        else std::swap(a[result], a[x]);
    } else if (before(a[x], a[z])) std::swap(a[result], a[x]);
    else if (before(a[y], a[z])) std::swap(a[result], a[z]);
    else std::swap(a[result], a[y]);
}

/* std::__introsort_loop.  skipBelow (larger-keys-first instances only): the part behind a cut holds keys <= the pivot's, so
 * when the pivot's key is below skipBelow that part is left as it is - its records keep their place relative to every record
 * outside it, only their order among themselves stays unsorted (the caller does not read it) */
ISR_TARGET static void intro_loop(rec_t* a, size_t first, size_t last, int depth, uint32_t skipBelow)
{
    while (last - first > 16) {
        if (depth == 0) {
            std::partial_sort(a + first, a + last, a + last, Before());      /* what std::sort itself calls here */
            return;
        }
        --depth;
        const size_t mid = first + (last - first) / 2;
        median_to_first(a, first, first + 1, mid, last - 1);
        const uint32_t pk = key_of(a[first]);
        const size_t cut = hoare_cut(a, first + 1, last, pk);
        if (!(ISR_DESC && pk < skipBelow)) intro_loop(a, cut, last, depth, skipBelow);
        last = cut;
    }
}

/* a[0..n) as std::__introsort_loop leaves it (depth limit 2 lg n unless overridden) */
ISR_TARGET static void partition_phase(rec_t* a, size_t n, int depthOverride, uint32_t skipBelow = 0)
{
    int lg = 0;
    for (size_t v = n; v > 1; v >>= 1) lg++;
    intro_loop(a, 0, n, depthOverride >= 0 ? depthOverride : 2 * lg, skipBelow);
}

#if !ISR_AVX2
/* std::__final_insertion_sort as one plain insertion sort (a record moves left past records it goes before: stable) */
static inline void insertion_pass(rec_t* a, size_t n)
{
    const Before before;
    for (size_t k = 1; k < n; k++) {
        const rec_t v = a[k];
        size_t p = k;
        while (p > 0 && before(v, a[p - 1])) { a[p] = a[p - 1]; p--; }
        a[p] = v;
    }
}

/* the plain transcription of std::__introsort_loop / std::__final_insertion_sort with a settable depth limit: the checker of
 * the heap-sort branch in tests (at the natural depth limit it is compared with std::sort itself).  *longestHeap = the longest range
 * that ran out of depth and went to std::__partial_sort, 0 if none did */
static inline void reference_sort(rec_t* a, size_t n, int depthOverride, size_t* longestHeap = nullptr)
{
    const Before before;
    struct R {
        static size_t partition(rec_t* a, size_t first, size_t last, size_t pivot, const Before& before)
        {
            for (;;) {
                while (before(a[first], a[pivot])) ++first;
                --last;
                while (before(a[pivot], a[last])) --last;
                if (!(first < last)) return first;
                std::swap(a[first], a[last]);
                ++first;
            }
        }
        static void loop(rec_t* a, size_t first, size_t last, int depth, const Before& before, size_t* longestHeap)
        {
            while (last - first > 16) {
                if (depth == 0) {
                    if (longestHeap && last - first > *longestHeap) *longestHeap = last - first;
                    std::partial_sort(a + first, a + last, a + last, before);
                    return;
                }
                --depth;
                median_to_first(a, first, first + 1, first + (last - first) / 2, last - 1);
                const size_t cut = partition(a, first + 1, last, first, before);
                loop(a, cut, last, depth, before, longestHeap);
                last = cut;
            }
        }
    };
    if (longestHeap) *longestHeap = 0;
    if (n < 2) return;
    int lg = 0;
    for (size_t v = n; v > 1; v >>= 1) lg++;
    R::loop(a, 0, n, depthOverride >= 0 ? depthOverride : 2 * lg, before, longestHeap);
    insertion_pass(a, n);
}
#endif

}  // namespace ISR_NS
