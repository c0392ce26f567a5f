// gsm_schedule_key.h -- what the Global renderer's blend-unit costs belong to (host only, plain C++17: no HIP).
// The blend orders its units by the walks the previous frame of the same key measured; a frame of another key
// starts from cleared costs.  A key is a vector of whole words, one field per word, compared word for word, so two
// frames that differ in any field differ in their keys.  DESIGN.md 6.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gsm {

// The kind of a Global frame: which projection, scatter and blend run, and which payload of the request is live.
enum class FrameKind : uint32_t {
    Single,   // one scene, one camera, the handle's tile rows (render, pick, occluded, styled)
    Records,  // a slab of received splat records in place of a projection (multi-GPU); its units are Single's
    Views,    // several cameras of one scene, one size (render_views)
    Batch,    // views of different scenes and sizes (render_batch)
    Compose,  // several posed objects in one target (render_composite and its pick / occluded / styled entries)
};

struct ScheduleKey {
    enum Word : size_t {
        kKind, kPick, kOccluded, kStyled, kUnitsPerTile, kWidth, kHeight, kRowBegin, kRowEnd, kRowStride,
        kViewCount,  // views of a Views / Batch frame, objects of a Compose frame, else 0
        kFixedWords  // then a Batch's (width, height, count) per view, or a Compose's count per object
    };
    // An orthographic frame (GSM_FRAME_ORTHOGRAPHIC; a Batch: any of its views) ends its key with one more word,
    // kOrthographicWord, after the tail (markOrthographic); a perspective frame's key has none.  The two therefore
    // differ in length whatever else they hold, so neither inherits the other's unit costs nor leaves it any -- the
    // rule that added kStyled -- and the keys of perspective frames are the words they were.
    static constexpr uint32_t kOrthographicWord = 1u;
    std::vector<uint32_t> words;
    ScheduleKey() : words(kFixedWords, 0u) { words.reserve(kFixedWords + 1); }
    void reserve(size_t n) { words.reserve(n); }
    // the fixed words zeroed but the kind, the tail dropped (no allocation)
    void reset(FrameKind kind) {
        words.assign(kFixedWords, 0u);
        words[kKind] = (uint32_t)kind;
    }
    uint32_t& operator[](Word w) { return words[w]; }
    uint32_t operator[](Word w) const { return words[w]; }
    void push(uint32_t w) { words.push_back(w); }
    // call last, after every tail word
    void markOrthographic() { words.push_back(kOrthographicWord); }
};

// The key the unit costs belong to (none before the first frame: every key differs from it).
class ScheduleState {
   public:
    ScheduleState() { words_.reserve(ScheduleKey::kFixedWords + 1); }  // (+ 1: the orthographic word)
    // room for keys of up to n words: no update() of such a key allocates afterwards
    void reserve(size_t n) { words_.reserve(n); }
    // adopts `key`; true when it differs from the stored one, i.e. the costs must be cleared
    bool update(const ScheduleKey& key) {
        if (words_ == key.words) return false;
        words_.assign(key.words.begin(), key.words.end());
        return true;
    }
    size_t capacity() const { return words_.capacity(); }
    const uint32_t* data() const { return words_.data(); }

   private:
    std::vector<uint32_t> words_;
};

}  // namespace gsm
