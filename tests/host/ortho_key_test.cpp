// ortho_key_test.cpp -- the schedule key's orthographic word (gsm_schedule_key.h) on the CPU: an
// orthographic frame neither inherits a perspective frame's blend-unit costs nor leaves it any, in every kind of
// frame; a perspective frame's key is the words it was; nothing allocates within a handle's reservation.  The
// request-side rule it restates is GlobalRenderer::requestKey's: every tail word first, the orthographic word last,
// a batch marked when any of its views is orthographic.
// Built and run by tests/test_ortho_key.py (g++ -std=c++17 -Wall -Wextra); that test also builds it with
// -fsanitize=address,undefined: this program is the stand-alone sanitizer target of the key code.
#include <cstdint>
#include <cstdio>
#include <vector>

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

struct View {
    uint32_t width, height, count;
    bool orthographic;
};

// requestKey's rule for a frame of `kind` with the given tail
static ScheduleKey frame_key(FrameKind kind, const std::vector<View>& views, bool frameOrthographic) {
    ScheduleKey k;
    k.reset(kind);
    k[ScheduleKey::kUnitsPerTile] = 2;
    k[ScheduleKey::kWidth] = 1920;
    k[ScheduleKey::kHeight] = 1080;
    k[ScheduleKey::kRowEnd] = 68;
    k[ScheduleKey::kRowStride] = 1;
    bool any = frameOrthographic;
    if (kind == FrameKind::Batch || kind == FrameKind::Compose) {
        k[ScheduleKey::kViewCount] = (uint32_t)views.size();
        for (const View& v : views) {
            if (kind == FrameKind::Batch) {
                k.push(v.width);
                k.push(v.height);
                any = any || v.orthographic;
            }
            k.push(v.count);
        }
    }
    if (any) k.markOrthographic();
    return k;
}

static bool clears_both_ways(const ScheduleKey& a, const ScheduleKey& b) {
    ScheduleState st;
    bool ok = st.update(a);
    ok = ok && !st.update(a);
    ok = ok && st.update(b);
    ok = ok && !st.update(b);
    ok = ok && st.update(a);
    return ok;
}

int main() {
    // a perspective frame's key is the words it was: kFixedWords of them, and the fixed words are unchanged
    CHECK(ScheduleKey::kFixedWords == 11);
    CHECK(frame_key(FrameKind::Single, {}, false).words.size() == ScheduleKey::kFixedWords);
    CHECK(frame_key(FrameKind::Single, {}, true).words.size() == ScheduleKey::kFixedWords + 1);
    CHECK(frame_key(FrameKind::Single, {}, true).words.back() == ScheduleKey::kOrthographicWord);
    // single, composite, batch: the orthographic frame and the perspective one clear each other's costs
    const std::vector<View> v3 = {{96, 48, 600, false}, {64, 32, 610, false}, {33, 17, 620, false}};
    for (FrameKind kind : {FrameKind::Single, FrameKind::Compose, FrameKind::Batch}) {
        const ScheduleKey p = frame_key(kind, v3, false), o = frame_key(kind, v3, true);
        CHECK(clears_both_ways(p, o));
        ScheduleState st;  // and each keeps its own costs from one frame to the next
        CHECK(st.update(o));
        CHECK(!st.update(frame_key(kind, v3, true)));
    }
    // a batch carries whether ANY view is orthographic: one orthographic view marks it, which one does not matter,
    // and the quad view (one perspective, three orthographic) keeps one key from frame to frame
    {
        std::vector<View> one = v3, other = v3, all = v3;
        one[0].orthographic = true;
        other[2].orthographic = true;
        for (View& v : all) v.orthographic = true;
        const ScheduleKey p = frame_key(FrameKind::Batch, v3, false);
        CHECK(clears_both_ways(p, frame_key(FrameKind::Batch, one, false)));
        ScheduleState st;
        CHECK(st.update(frame_key(FrameKind::Batch, one, false)));
        CHECK(!st.update(frame_key(FrameKind::Batch, other, false)));
        CHECK(!st.update(frame_key(FrameKind::Batch, all, false)));
        CHECK(st.update(p));
    }
    // the word cannot be mistaken for a tail word: a perspective composite of n + 1 objects whose last count is 1
    // against an orthographic composite of n objects (the view counts differ), and the same for a batch's tail
    {
        std::vector<View> v4 = v3;
        v4.push_back({0, 0, ScheduleKey::kOrthographicWord, false});
        CHECK(clears_both_ways(frame_key(FrameKind::Compose, v4, false), frame_key(FrameKind::Compose, v3, true)));
        ScheduleKey forged = frame_key(FrameKind::Compose, v3, false);
        forged.push(ScheduleKey::kOrthographicWord);  // (only markOrthographic appends it: the same key)
        ScheduleState st;
        CHECK(st.update(forged));
        CHECK(!st.update(frame_key(FrameKind::Compose, v3, true)));
    }
    // an orthographic frame differs from every other option's frame of the same size
    {
        const ScheduleKey o = frame_key(FrameKind::Single, {}, true);
        for (ScheduleKey::Word w : {ScheduleKey::kPick, ScheduleKey::kOccluded, ScheduleKey::kStyled}) {
            ScheduleKey k = frame_key(FrameKind::Single, {}, false);
            k[w] = 1;
            CHECK(clears_both_ways(o, k));
            ScheduleKey ko = frame_key(FrameKind::Single, {}, true);
            ko[w] = 1;
            CHECK(clears_both_ways(o, ko));
            CHECK(clears_both_ways(k, ko));
        }
    }
    // no allocation: a default key and a default state hold an orthographic Single key without growing, and a
    // handle's batch reservation (kFixedWords + 3 views + 1) holds an orthographic batch of that many views
    {
        ScheduleKey k;
        const uint32_t* const kdata = k.words.data();
        const size_t kcap = k.words.capacity();
        CHECK(kcap >= ScheduleKey::kFixedWords + 1);
        ScheduleState st;
        const uint32_t* const sdata = st.data();
        const size_t scap = st.capacity();
        for (int i = 0; i < 4; ++i) {
            k.reset(FrameKind::Single);
            if (i & 1) k.markOrthographic();
            CHECK(st.update(k) == true);
            CHECK(k.words.data() == kdata && k.words.capacity() == kcap);
            CHECK(st.data() == sdata && st.capacity() == scap);
        }
        const size_t views = 40, n = ScheduleKey::kFixedWords + 3 * views + 1;
        ScheduleKey b;
        b.reserve(n);
        ScheduleState bs;
        bs.reserve(n);
        const uint32_t* const bdata = b.words.data();
        const uint32_t* const bsdata = bs.data();
        for (int round = 0; round < 3; ++round) {
            b.reset(FrameKind::Batch);
            for (size_t i = 0; i < 3 * views; ++i) b.push((uint32_t)(i + round));
            b.markOrthographic();
            CHECK(b.words.size() == n);
            CHECK(bs.update(b));
            CHECK(b.words.data() == bdata && bs.data() == bsdata);
        }
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("orthographic schedule key: all checks passed\n");
    return 0;
}
