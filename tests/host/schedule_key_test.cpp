// schedule_key_test.cpp -- the Global renderer's schedule key (gsm_schedule_key.h) on the CPU: which frames share
// their blend-unit costs and which clear them, and that a stored key never allocates within its reservation.
// Built and run by tests/test_schedule_key.py (g++ -std=c++17 -Wall -Wextra); prints the failed checks, exits 1.
#include <cstdint>
#include <cstdio>

#include "gsm_schedule_key.h"

using gsm::FrameKind;
using gsm::ScheduleKey;
using gsm::ScheduleState;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// a 1080p single frame of a handle with 68 tile rows
static ScheduleKey base_key() {
    ScheduleKey k;
    k.reset(FrameKind::Single);
    k[ScheduleKey::kUnitsPerTile] = 2;
    k[ScheduleKey::kWidth] = 1920;
    k[ScheduleKey::kHeight] = 1080;
    k[ScheduleKey::kRowBegin] = 0;
    k[ScheduleKey::kRowEnd] = 68;
    k[ScheduleKey::kRowStride] = 1;
    return k;
}

// `b` after `a` clears, `b` again does not, and `a` after `b` clears again
static bool clears_both_ways(const ScheduleKey& a, const ScheduleKey& b) {
    ScheduleState st;
    bool ok = st.update(a);  // (the first frame of a handle clears)
    ok = ok && !st.update(a);
    ok = ok && st.update(b);
    ok = ok && !st.update(b);
    ok = ok && st.update(a);
    return ok;
}

// the single-frame key this header replaced: a 64-bit XOR of shifted fields whose ranges overlap
static uint64_t legacy_xor_key(uint32_t upt, uint32_t width, uint32_t height, uint32_t stride, uint32_t begin,
                               uint32_t end) {
    return ((uint64_t)upt << 60) ^ ((uint64_t)width << 40) ^ ((uint64_t)height << 20) ^ ((uint64_t)stride << 30) ^
           ((uint64_t)begin << 10) ^ end;
}

static ScheduleKey batch_key(const uint32_t (*views)[3], uint32_t n) {
    ScheduleKey k = base_key();
    k[ScheduleKey::kKind] = (uint32_t)FrameKind::Batch;
    k[ScheduleKey::kViewCount] = n;
    for (uint32_t v = 0; v < n; ++v)
        for (uint32_t j = 0; j < 3; ++j) k.push(views[v][j]);
    return k;
}

static ScheduleKey compose_key(const uint32_t* counts, uint32_t n) {
    ScheduleKey k = base_key();
    k[ScheduleKey::kKind] = (uint32_t)FrameKind::Compose;
    k[ScheduleKey::kViewCount] = n;
    for (uint32_t o = 0; o < n; ++o) k.push(counts[o]);
    return k;
}

int main() {
    // the same key twice: no clear
    {
        ScheduleState st;
        CHECK(st.update(base_key()));
        CHECK(!st.update(base_key()));
        CHECK(!st.update(base_key()));
    }
    // exactly one field changed: a clear, either way round
    {
        const ScheduleKey::Word fields[] = {
            ScheduleKey::kKind,   ScheduleKey::kPick,     ScheduleKey::kOccluded, ScheduleKey::kStyled,
            ScheduleKey::kUnitsPerTile, ScheduleKey::kWidth, ScheduleKey::kHeight, ScheduleKey::kRowBegin,
            ScheduleKey::kRowEnd, ScheduleKey::kRowStride, ScheduleKey::kViewCount};
        static_assert(sizeof(fields) / sizeof(fields[0]) == ScheduleKey::kFixedWords, "every fixed word");
        for (ScheduleKey::Word f : fields) {
            ScheduleKey k = base_key();
            k[f] += 1;
            CHECK(clears_both_ways(base_key(), k));
        }
        // every kind differs from every other
        for (uint32_t a = 0; a < 5; ++a)
            for (uint32_t b = a + 1; b < 5; ++b) {
                ScheduleKey ka = base_key(), kb = base_key();
                ka[ScheduleKey::kKind] = a;
                kb[ScheduleKey::kKind] = b;
                CHECK(clears_both_ways(ka, kb));
            }
    }
    // a batch signature: one changed width, height or count of the middle view; a fourth view
    {
        const uint32_t v3[3][3] = {{96, 48, 600}, {64, 32, 610}, {33, 17, 620}};
        const ScheduleKey k3 = batch_key(v3, 3);
        for (uint32_t j = 0; j < 3; ++j) {
            uint32_t w[3][3];
            for (uint32_t v = 0; v < 3; ++v)
                for (uint32_t i = 0; i < 3; ++i) w[v][i] = v3[v][i];
            w[1][j] += 1;
            CHECK(clears_both_ways(k3, batch_key(w, 3)));
        }
        const uint32_t v4[4][3] = {{96, 48, 600}, {64, 32, 610}, {33, 17, 620}, {33, 17, 620}};
        CHECK(clears_both_ways(k3, batch_key(v4, 4)));
        // (the same tail words under one more view count, and one more view under the same count)
        ScheduleKey sameTail = k3;
        sameTail[ScheduleKey::kViewCount] = 4;
        CHECK(clears_both_ways(k3, sameTail));
        ScheduleKey sameCount = batch_key(v4, 4);
        sameCount[ScheduleKey::kViewCount] = 3;
        CHECK(clears_both_ways(k3, sameCount));
    }
    // a composite: one changed count, a fourth object (an empty one included)
    {
        const uint32_t c3[3] = {600, 0, 620};
        const ScheduleKey k3 = compose_key(c3, 3);
        for (uint32_t o = 0; o < 3; ++o) {
            uint32_t c[3] = {c3[0], c3[1], c3[2]};
            c[o] += 1;
            CHECK(clears_both_ways(k3, compose_key(c, 3)));
        }
        const uint32_t c4[4] = {600, 0, 620, 0};
        CHECK(clears_both_ways(k3, compose_key(c4, 4)));
        // a composite never shares with a batch of the same words
        ScheduleKey asBatch = k3;
        asBatch[ScheduleKey::kKind] = (uint32_t)FrameKind::Batch;
        CHECK(clears_both_ways(k3, asBatch));
    }
    // the pairs the replaced XOR key could not tell apart
    {
        const uint32_t hs[] = {1080, 2160, 4096, 1024};
        for (uint32_t h : hs) {
            CHECK(legacy_xor_key(2, 1920, h, 1, 0, 68) == legacy_xor_key(2, 1920, h ^ 3072u, 2, 0, 68));
            ScheduleKey a = base_key(), b = base_key();
            a[ScheduleKey::kHeight] = h;
            a[ScheduleKey::kRowStride] = 1;
            b[ScheduleKey::kHeight] = h ^ 3072u;
            b[ScheduleKey::kRowStride] = 2;
            CHECK(clears_both_ways(a, b));
        }
        const uint32_t es[] = {68, 1030, 2047, 4096};
        for (uint32_t e : es) {
            CHECK(legacy_xor_key(2, 1920, 1080, 1, 1, e) == legacy_xor_key(2, 1920, 1080, 1, 0, e ^ 1024u));
            ScheduleKey a = base_key(), b = base_key();
            a[ScheduleKey::kRowBegin] = 1;
            a[ScheduleKey::kRowEnd] = e;
            b[ScheduleKey::kRowBegin] = 0;
            b[ScheduleKey::kRowEnd] = e ^ 1024u;
            CHECK(clears_both_ways(a, b));
        }
    }
    // no allocation within the reservation: keys of up to n words move neither the stored copy nor the working key
    {
        const size_t n = ScheduleKey::kFixedWords + 3 * 40;
        ScheduleState st;
        st.reserve(n);
        ScheduleKey k;
        k.reserve(n);
        const size_t cap = st.capacity(), kcap = k.words.capacity();
        const uint32_t* const data = st.data();
        const uint32_t* const kdata = k.words.data();
        CHECK(cap >= n && kcap >= n);
        const size_t sizes[] = {ScheduleKey::kFixedWords, n, ScheduleKey::kFixedWords + 1, n - 1, n,
                                ScheduleKey::kFixedWords};
        uint32_t salt = 0;
        for (size_t words : sizes) {
            k.reset(FrameKind::Batch);
            while (k.words.size() < words) k.push(++salt);
            CHECK(k.words.size() == words);
            CHECK(st.update(k));
            CHECK(!st.update(k));
            CHECK(st.capacity() == cap && st.data() == data);
            CHECK(k.words.capacity() == kcap && k.words.data() == kdata);
        }
        // (a default state holds a Single / Views / Records key without growing)
        ScheduleState small;
        const size_t scap = small.capacity();
        const uint32_t* const sdata = small.data();
        CHECK(scap >= ScheduleKey::kFixedWords);
        CHECK(small.update(base_key()));
        CHECK(small.capacity() == scap && small.data() == sdata);
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("schedule key: all checks passed\n");
    return 0;
}
