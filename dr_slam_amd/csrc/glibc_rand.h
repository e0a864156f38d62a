/* glibc_rand.h — glibc's rand() restated as a stream of one's own, and DUtils::Random::RandomInt on top of it.
 *
 * rand() is process-wide in the reference and shared between its threads, so what a RANSAC draws depends on who drew before
 * (SURVEY.md §9.3).  Every consumer here (drfe_lines_is_good, the Sim3 solver) owns a GlibcRand seeded by its caller instead; the
 * numbers are those srand(seed) followed by rand() gives on glibc.  Host code. */
#ifndef DRFE_GLIBC_RAND_H
#define DRFE_GLIBC_RAND_H

#include <stdint.h>

/* glibc random_r TYPE_3 (x^31 + x^3 + 1), what rand() runs: r[i] = r[i-31] + r[i-3], output >> 1; the seed
 * expands through the 16807 Lehmer step and the first 310 outputs are discarded. */
struct GlibcRand {
    uint32_t r[34];
    int pos;
    explicit GlibcRand(uint32_t seed)
    {
        uint32_t t[344];
        int32_t w = seed ? (int32_t)seed : 1;
        t[0] = (uint32_t)w;
        for (int i = 1; i < 31; i++) {
            const int32_t hi = w / 127773, lo = w % 127773;
            w = 16807 * lo - 2836 * hi;
            if (w < 0) w += 2147483647;
            t[i] = (uint32_t)w;
        }
        for (int i = 31; i < 34; i++) t[i] = t[i - 31];
        for (int i = 34; i < 344; i++) t[i] = t[i - 31] + t[i - 3];
        for (int i = 0; i < 34; i++) r[i] = t[310 + i];   /* the last 34 values: enough history for i-31 */
        pos = 0;
    }
    int next()
    {
        /* ring of 34: newest at (pos+33)%34; r[i-31] is 31 back from the new element, r[i-3] three back */
        const uint32_t v = r[(pos + 34 - 31) % 34] + r[(pos + 34 - 3) % 34];
        r[pos] = v;
        pos = (pos + 1) % 34;
        return (int)(v >> 1);
    }
    /* DUtils::Random::RandomInt(min, max) (reference Thirdparty/DBoW2/DUtils/Random.cpp:47-50), RAND_MAX = 2^31 - 1 */
    int random_int(int min, int max)
    {
        const int d = max - min + 1;
        return (int)(((double)next() / (2147483647.0 + 1.0)) * d) + min;
    }
};

#endif
