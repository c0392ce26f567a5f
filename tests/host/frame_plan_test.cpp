// frame_plan_test.cpp -- the Global frame entries' admission rows and layouts (gsm_frame_plan.h) on the CPU: what each
// entry refuses and in which order, and where every view and object lies in the handle's item and tile space.  Every
// expected status and number below is a literal written by hand from the entries' documented rows (never computed by
// the functions under test).  The handle is small so that every boundary is reachable: max_gaussians 1024 (4 blocks
// of 256), 64 x 32 pixels (2 x 2 tiles of 32 x 16), RGBA16F (8 bytes a pixel).  Addresses are never dereferenced.
// Built and run by tests/test_frame_plan.py (g++ -std=c++17 -Wall -Wextra -Werror); prints the failed rows, exits 1.
#include <cstdint>
#include <cstdio>
#include <deque>
#include <vector>

#include "gsm_frame_plan.h"

using namespace gsm;

static int failures = 0, checks = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        ++checks;                                                 \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)
static void expect_status(int line, const char* what, gsm_status got, gsm_status want) {
    ++checks;
    if (got == want) return;
    ++failures;
    std::printf("FAILED line %d: %s = %d, expected %d\n", line, what, (int)got, (int)want);
}
#define ST(expr, want) expect_status(__LINE__, #expr, (expr), (want))

constexpr gsm_status OK = GSM_OK, COUNT = GSM_ERR_INVALID_GAUSSIAN_COUNT, DIM = GSM_ERR_INVALID_DIMENSIONS,
                     SIZE = GSM_ERR_INVALID_BUFFER_SIZE, TILES = GSM_ERR_INVALID_TILE_COUNT,
                     MISSING = GSM_ERR_MISSING_REQUIRED_BUFFER, ARG = GSM_ERR_INVALID_ARGUMENT,
                     UNSUP = GSM_ERR_UNSUPPORTED;

static void* P(uintptr_t a) { return (void*)a; }

static FrameLimits small() {
    FrameLimits L;
    L.colorFormat = GSM_COLOR_FORMAT_RGBA16F;
    L.maxGaussians = 1024;
    L.maxWidth = 64;
    L.maxHeight = 32;
    L.tileCount = 4;
    L.tilesY = 2;
    return L;
}
// a handle whose tile space and item space lie above the 16-bit bound
static FrameLimits large() {
    FrameLimits L = small();
    L.maxGaussians = 30000000;
    L.tileCount = 70000;
    return L;
}
static FrameLimits restricted() {
    FrameLimits L = small();
    L.rowsRestricted = true;
    return L;
}
static gsm_gaussian_input scene(uint32_t count, uint32_t sh = 1) {
    gsm_gaussian_input in{};
    in.gaussians = P(0x10000);
    in.harmonics = P(0x20000);
    in.gaussian_count = count;
    in.sh_components = sh;
    return in;
}
// targets of a 64-pixel row: colour 512 bytes, depth 128, pick and occluder 256
static FrameTargets targets() { return FrameTargets{P(0x1000), 512, P(0x2000), 128}; }
static const gsm_global_state kState[2] = {{nullptr, 0, 0}, {nullptr, 255, 0}};
static gsm_global_style kStyles[256];

static void test_rules() {
    CHECK(kProjectBlock == 256 && kStyleEntries == 256 && kMaxSlabs == 16 && kBatchIndexMax == 65535);
    CHECK(kTileWidth == 32 && kTileHeight == 16);
    CHECK(blocks_of(0) == 0 && blocks_of(1) == 1 && blocks_of(256) == 1 && blocks_of(257) == 2 && blocks_of(1024) == 4);
    CHECK(blocks_of(0xFFFFFFFFu) == 16777216u);
    CHECK(padded_items(0) == 0 && padded_items(1) == 256 && padded_items(256) == 256 && padded_items(257) == 512);
    CHECK(padded_items(1024) == 1024 && padded_items(0xFFFFFFFFu) == 4294967296ull);
    CHECK(tiles_x(1) == 1 && tiles_x(32) == 1 && tiles_x(33) == 2 && tiles_x(64) == 2 && tiles_x(65) == 3);
    CHECK(tiles_y(1) == 1 && tiles_y(16) == 1 && tiles_y(17) == 2 && tiles_y(32) == 2 && tiles_y(33) == 3);
    CHECK(tiles_of(1, 1) == 1 && tiles_of(32, 16) == 1 && tiles_of(33, 17) == 4 && tiles_of(64, 32) == 4);
    CHECK(tiles_of(1920, 1080) == 4080);
    CHECK(max_batch_views(4) == 4 && max_batch_views(65535) == 65535 && max_batch_views(65536) == 65535);
    CHECK(max_batch_views(70000) == 65535 && max_batch_views(1) == 1);
    CHECK(max_compose_entries(4) == 4 && max_compose_entries(65536) == 65535 && max_compose_entries(117188) == 65535);
    CHECK(batch_tiles_ok(4, 4) && !batch_tiles_ok(5, 4) && batch_tiles_ok(0, 4));
    CHECK(batch_tiles_ok(65535, 70000) && !batch_tiles_ok(65536, 70000) && !batch_tiles_ok(1ull << 33, 70000));
    CHECK(color_bytes_per_pixel(GSM_COLOR_FORMAT_RGBA16F) == 8 && color_bytes_per_pixel(GSM_COLOR_FORMAT_RGBA32F) == 16);
    CHECK(color_bytes_per_pixel(GSM_COLOR_FORMAT_RGBA8_UNORM) == 4 && color_bytes_per_pixel(GSM_COLOR_FORMAT_BGRA8_UNORM_SRGB) == 4);
    FrameLimits L = small();
    CHECK(L.maxBlocks() == 4);
    L.maxGaussians = 1025;
    CHECK(L.maxBlocks() == 5);
    L.maxGaussians = 30000000;
    CHECK(L.maxBlocks() == 117188);
    L = small();
    CHECK(L.sizeOk(1, 1) && L.sizeOk(64, 32) && !L.sizeOk(0, 1) && !L.sizeOk(1, 0) && !L.sizeOk(65, 32) && !L.sizeOk(64, 33));
}

// validate_frame as the DepthFirst and Local renderers call it, and through the config
static void test_validate_frame() {
    gsm_renderer_config cfg{};
    cfg.color_format = GSM_COLOR_FORMAT_RGBA16F;
    ST(validate_frame(cfg, 1024, 64, 32, 100, false, false, 64, 32, P(0x1000), 512, 1, P(0x2000), 128), OK);
    ST(validate_frame(cfg, 1024, 64, 32, 0, false, false, 64, 32, P(0x1000), 512, 1, P(0x2000), 128), COUNT);  // !allowEmpty
    ST(validate_frame(cfg, 1024, 64, 32, 0, true, true, 64, 32, P(0x1000), 512, 1, P(0x2000), 128), OK);
    ST(validate_frame(cfg, 1024, 64, 32, 1, true, true, 64, 32, P(0x1000), 512, 1, P(0x2000), 128), MISSING);
    // side by side: a row holds two frames
    ST(validate_frame(cfg, 1024, 64, 32, 1, false, false, 64, 32, P(0x1000), 1024, 2, nullptr, 0), OK);
    ST(validate_frame(cfg, 1024, 64, 32, 1, false, false, 64, 32, P(0x1000), 1020, 2, nullptr, 0), SIZE);
    cfg.color_format = GSM_COLOR_FORMAT_RGBA32F;
    ST(validate_frame(cfg, 1024, 64, 32, 1, false, false, 64, 32, P(0x1000), 1024, 1, nullptr, 0), OK);
    ST(validate_frame(cfg, 1024, 64, 32, 1, false, false, 64, 32, P(0x1000), 1020, 1, nullptr, 0), SIZE);
    cfg.color_format = GSM_COLOR_FORMAT_BGRA8_UNORM_SRGB;
    ST(validate_frame(cfg, 1024, 64, 32, 1, false, false, 64, 32, P(0x1000), 256, 1, nullptr, 0), OK);
    ST(validate_frame(cfg, 1024, 64, 32, 1, false, false, 64, 32, P(0x1000), 252, 1, nullptr, 0), SIZE);
}

static void test_single_frame() {
    const FrameLimits L = small();
    const FrameTargets t = targets();
    const FrameExtras none;
    const PickTarget pick{P(0x3000), 256};
    const OccluderSource occ{P(0x4000), 256};
    const StyleSource style{kState, kStyles, 3};
    FrameExtras withPick, withOcc, withStyle, ortho, all;
    withPick.pick = all.pick = &pick;
    withOcc.occluder = all.occluder = &occ;
    withStyle.style = all.style = &style;
    ortho.orthographic = all.orthographic = true;
    ST(check_frame(L, scene(100), 64, 32, t, none), OK);
    ST(check_frame(L, scene(100), 64, 32, t, all), OK);
    ST(check_frame(L, scene(100), 1, 1, t, none), OK);
    // counts 0, 1, 256, 257, max and one past it; an empty scene needs no input
    for (uint32_t n : {0u, 1u, 256u, 257u, 1024u}) ST(check_frame(L, scene(n), 64, 32, t, none), OK);
    ST(check_frame(L, scene(1025), 64, 32, t, none), COUNT);
    gsm_gaussian_input in = scene(0);
    in.gaussians = in.harmonics = nullptr;
    ST(check_frame(L, in, 64, 32, t, none), OK);
    // dimensions
    ST(check_frame(L, scene(1), 0, 32, t, none), DIM);
    ST(check_frame(L, scene(1), 64, 0, t, none), DIM);
    ST(check_frame(L, scene(1), 65, 32, t, none), DIM);
    ST(check_frame(L, scene(1), 64, 33, t, none), DIM);
    // missing buffers
    FrameTargets bad = t;
    bad.color = nullptr;
    ST(check_frame(L, scene(1), 64, 32, bad, none), MISSING);
    in = scene(1);
    in.gaussians = nullptr;
    ST(check_frame(L, in, 64, 32, t, none), MISSING);
    in = scene(1);
    in.harmonics = nullptr;
    ST(check_frame(L, in, 64, 32, t, none), MISSING);
    const PickTarget noPick{nullptr, 256};
    const OccluderSource noOcc{nullptr, 256};
    FrameExtras e;
    e.pick = &noPick;
    ST(check_frame(L, scene(1), 64, 32, t, e), MISSING);
    e = none;
    e.occluder = &noOcc;
    ST(check_frame(L, scene(1), 64, 32, t, e), MISSING);
    // sizes: the colour pitch one byte short (and so misaligned), a whole word short, misaligned alone; the pointer
    // off by 1 and by 2
    for (size_t pitch : {511u, 508u, 514u, 513u}) {
        bad = t;
        bad.colorPitch = pitch;
        ST(check_frame(L, scene(1), 64, 32, bad, none), SIZE);
    }
    bad = t;
    bad.colorPitch = 516;
    ST(check_frame(L, scene(1), 64, 32, bad, none), OK);
    for (uintptr_t a : {0x1001u, 0x1002u, 0x1003u}) {
        bad = t;
        bad.color = P(a);
        ST(check_frame(L, scene(1), 64, 32, bad, none), SIZE);
    }
    bad = t;
    bad.color = P(0x1004);
    ST(check_frame(L, scene(1), 64, 32, bad, none), OK);
    // depth: null is no depth (its pitch is not read), short, odd, the pointer off by 1 (by 2: aligned)
    bad = t;
    bad.depth = nullptr;
    bad.depthPitch = 1;
    ST(check_frame(L, scene(1), 64, 32, bad, none), OK);
    for (size_t pitch : {126u, 127u, 129u}) {
        bad = t;
        bad.depthPitch = pitch;
        ST(check_frame(L, scene(1), 64, 32, bad, none), SIZE);
    }
    bad = t;
    bad.depthPitch = 130;
    ST(check_frame(L, scene(1), 64, 32, bad, none), OK);
    bad = t;
    bad.depth = P(0x2001);
    ST(check_frame(L, scene(1), 64, 32, bad, none), SIZE);
    bad.depth = P(0x2002);
    ST(check_frame(L, scene(1), 64, 32, bad, none), OK);
    // a 32-pixel frame needs half the pitches
    ST(check_frame(L, scene(1), 32, 16, FrameTargets{P(0x1000), 256, P(0x2000), 64}, none), OK);
    ST(check_frame(L, scene(1), 33, 16, FrameTargets{P(0x1000), 256, P(0x2000), 66}, none), SIZE);
    ST(check_frame(L, scene(1), 33, 16, FrameTargets{P(0x1000), 264, P(0x2000), 64}, none), SIZE);
    // pick and occluder: pitch short, misaligned, pixels off by 1 and by 2
    for (size_t pitch : {252u, 255u, 258u}) {
        const PickTarget p{P(0x3000), pitch};
        const OccluderSource o{P(0x4000), pitch};
        e = none;
        e.pick = &p;
        ST(check_frame(L, scene(1), 64, 32, t, e), SIZE);
        e = none;
        e.occluder = &o;
        ST(check_frame(L, scene(1), 64, 32, t, e), SIZE);
    }
    for (uintptr_t off : {1u, 2u, 3u}) {
        const PickTarget p{P(0x3000 + off), 256};
        const OccluderSource o{P(0x4000 + off), 256};
        e = none;
        e.pick = &p;
        ST(check_frame(L, scene(1), 64, 32, t, e), SIZE);
        e = none;
        e.occluder = &o;
        ST(check_frame(L, scene(1), 64, 32, t, e), SIZE);
    }
    {
        const PickTarget p{P(0x3004), 260};
        const OccluderSource o{P(0x4004), 260};
        e = none;
        e.pick = &p;
        e.occluder = &o;
        ST(check_frame(L, scene(1), 64, 32, t, e), OK);
    }
    // the styled row: style count 0, 256, 257; a null table; null states; default_state 255 and 256
    StyleSource s = style;
    s.styleCount = 0;
    e = none;
    e.style = &s;
    ST(check_frame(L, scene(1), 64, 32, t, e), ARG);
    s.styleCount = 257;
    ST(check_frame(L, scene(1), 64, 32, t, e), ARG);
    s.styleCount = 256;
    ST(check_frame(L, scene(1), 64, 32, t, e), OK);
    s.styleCount = 1;
    ST(check_frame(L, scene(1), 64, 32, t, e), OK);
    s = style;
    s.styles = nullptr;
    ST(check_frame(L, scene(1), 64, 32, t, e), ARG);
    s = style;
    s.states = nullptr;
    ST(check_frame(L, scene(1), 64, 32, t, e), ARG);
    gsm_global_state st{nullptr, 256, 0};
    s = style;
    s.states = &st;
    ST(check_frame(L, scene(1), 64, 32, t, e), ARG);
    st.default_state = 255;
    ST(check_frame(L, scene(1), 64, 32, t, e), OK);
    // the tile-rows row: each of pick, occluder, style and the orthographic flag alone is refused; the plain frame
    // is a restricted handle's own
    const FrameLimits R = restricted();
    ST(check_frame(R, scene(100), 64, 32, t, none), OK);
    ST(check_frame(R, scene(100), 64, 32, t, withPick), UNSUP);
    ST(check_frame(R, scene(100), 64, 32, t, withOcc), UNSUP);
    ST(check_frame(R, scene(100), 64, 32, t, withStyle), UNSUP);
    ST(check_frame(R, scene(100), 64, 32, t, ortho), UNSUP);
    // interleaved rows come from the records path only
    FrameLimits R2 = restricted();
    R2.rowStride = 2;
    ST(check_frame(R2, scene(100), 64, 32, t, none), ARG);
    // two rows failing at once: the earlier decides
    bad = t;
    bad.color = nullptr;
    ST(check_frame(L, scene(1025), 0, 32, t, none), COUNT);      // count, dimensions
    ST(check_frame(L, scene(1), 65, 32, bad, none), DIM);        // dimensions, missing buffer
    bad.depthPitch = 127;
    ST(check_frame(L, scene(1), 64, 32, bad, none), MISSING);    // missing buffer, size
    bad = t;
    bad.colorPitch = 508;
    s = style;
    s.styleCount = 0;
    ST(check_frame(L, scene(1), 64, 32, bad, e), SIZE);          // size, style
    ST(check_frame(R, scene(1), 64, 32, t, e), ARG);             // style, tile rows
    ST(check_frame(R2, scene(1), 64, 32, t, withPick), UNSUP);   // tile rows, row stride
}

static void test_views() {
    const FrameLimits L = small();
    const gsm_camera_params* cams = (const gsm_camera_params*)P(0x5000);
    // 32 x 16 views: one tile each; rows of 256 bytes, 16 rows a view
    const FrameTargets t{P(0x1000), 256, P(0x2000), 64};
    const size_t cs = 4096, ds = 1024;
    ST(check_views(L, scene(256), cams, 4, 32, 16, t, cs, ds), OK);  // items exactly max, tiles exactly the handle's
    ST(check_views(L, scene(1), cams, 4, 32, 16, t, cs, ds), OK);
    ST(check_views(L, scene(0), cams, 4, 32, 16, t, cs, ds), OK);
    ST(check_views(L, scene(257), cams, 2, 32, 16, t, cs, ds), OK);      // 2 x 512 items
    ST(check_views(L, scene(257), cams, 3, 32, 16, t, cs, ds), COUNT);   // 3 x 512 items, although 771 gaussians fit
    ST(check_views(L, scene(1024), cams, 1, 32, 16, t, cs, ds), OK);
    ST(check_views(L, scene(1024), cams, 2, 32, 16, t, cs, ds), COUNT);
    ST(check_views(L, scene(1025), cams, 1, 32, 16, t, cs, ds), COUNT);
    ST(check_views(L, scene(1), cams, 0, 32, 16, t, cs, ds), COUNT);
    ST(check_views(L, scene(1), cams, 5, 32, 16, t, cs, ds), COUNT);     // one block past max
    ST(check_views(L, scene(1), cams, 1, 0, 16, t, cs, ds), DIM);
    ST(check_views(L, scene(1), cams, 1, 65, 16, t, cs, ds), DIM);
    ST(check_views(L, scene(1), cams, 1, 32, 33, t, cs, ds), DIM);
    ST(check_views(L, scene(0), cams, 5, 32, 16, t, cs, ds), TILES);     // one tile past the handle's
    ST(check_views(L, scene(0), cams, 2, 33, 16, t, 8192, 2048), SIZE);  // (4 tiles pass; the 33-pixel row does not fit)
    ST(check_views(L, scene(0), cams, 2, 33, 17, FrameTargets{P(0x1000), 264, P(0x2000), 66}, 8192, 2048), TILES);
    const FrameLimits B = large();
    ST(check_views(B, scene(0), cams, 65535, 32, 16, t, cs, ds), OK);
    ST(check_views(B, scene(0), cams, 65536, 32, 16, t, cs, ds), TILES);
    // view_count * tiles = 2^31 * 4 is 0 in 32 bits
    ST(check_views(B, scene(0), cams, 0x80000000u, 64, 32, FrameTargets{P(0x1000), 512, nullptr, 0}, 16384, 0), TILES);
    ST(check_views(L, scene(1), nullptr, 1, 32, 16, t, cs, ds), MISSING);
    FrameTargets bad = t;
    bad.color = nullptr;
    ST(check_views(L, scene(1), cams, 1, 32, 16, bad, cs, ds), MISSING);
    gsm_gaussian_input in = scene(1);
    in.harmonics = nullptr;
    ST(check_views(L, in, cams, 1, 32, 16, t, cs, ds), MISSING);
    bad = t;
    bad.colorPitch = 252;
    ST(check_views(L, scene(1), cams, 1, 32, 16, bad, cs, ds), SIZE);
    bad = t;
    bad.depthPitch = 63;
    ST(check_views(L, scene(1), cams, 1, 32, 16, bad, cs, ds), SIZE);
    // view strides: short, misaligned (colour 4 bytes, depth 2); without depth its stride is not read
    ST(check_views(L, scene(1), cams, 2, 32, 16, t, 4092, ds), SIZE);
    ST(check_views(L, scene(1), cams, 2, 32, 16, t, 4098, ds), SIZE);
    ST(check_views(L, scene(1), cams, 2, 32, 16, t, 4100, ds), OK);
    ST(check_views(L, scene(1), cams, 2, 32, 16, t, cs, 1022), SIZE);
    ST(check_views(L, scene(1), cams, 2, 32, 16, t, cs, 1025), SIZE);
    ST(check_views(L, scene(1), cams, 2, 32, 16, t, cs, 1026), OK);
    ST(check_views(L, scene(1), cams, 2, 32, 16, FrameTargets{P(0x1000), 256, nullptr, 0}, cs, 1), OK);
    ST(check_views(restricted(), scene(1), cams, 2, 32, 16, t, cs, ds), UNSUP);
    // two rows at once
    ST(check_views(L, scene(1025), cams, 1, 65, 16, t, cs, ds), COUNT);           // count, dimensions
    ST(check_views(L, scene(0), cams, 5, 65, 16, t, cs, ds), DIM);                // dimensions, tiles
    ST(check_views(L, scene(0), nullptr, 5, 32, 16, t, cs, ds), TILES);           // tiles, missing buffer
    bad = t;
    bad.colorPitch = 252;
    ST(check_views(L, scene(1), nullptr, 1, 32, 16, bad, cs, ds), MISSING);       // missing buffer, size
    ST(check_views(restricted(), scene(1), cams, 2, 32, 16, t, 4092, ds), SIZE);  // size, tile rows
    // the layout
    ViewsLayout v = views_layout(0, 1, 1);
    CHECK(v.blocksPerView == 0 && v.tilesPerView == 1);
    v = views_layout(1, 32, 16);
    CHECK(v.blocksPerView == 1 && v.tilesPerView == 1);
    v = views_layout(256, 33, 17);
    CHECK(v.blocksPerView == 1 && v.tilesPerView == 4);
    v = views_layout(257, 64, 32);
    CHECK(v.blocksPerView == 2 && v.tilesPerView == 4);
    v = views_layout(1000000, 1920, 1080);
    CHECK(v.blocksPerView == 3907 && v.tilesPerView == 4080);
}

static gsm_global_view view(uint32_t count, uint32_t w = 32, uint32_t h = 16) {
    gsm_global_view V{};
    V.input = scene(count);
    V.width = w;
    V.height = h;
    V.color = P(0x1000);
    V.color_pitch_bytes = 512;
    V.depth = P(0x2000);
    V.depth_pitch_bytes = 128;
    return V;
}
static gsm_status batch(const FrameLimits& L, const std::vector<gsm_global_view>& v,
                        const std::vector<BatchViewOptions>* o = nullptr) {
    return check_batch(L, BatchViewArray{v.data(), o ? o->data() : nullptr}, (uint32_t)v.size());
}

static void test_batch() {
    const FrameLimits L = small();
    using Views = std::vector<gsm_global_view>;
    ST(check_batch(L, BatchViewArray{nullptr, nullptr}, 0), COUNT);  // (both: the count row is first)
    ST(check_batch(L, BatchViewArray{nullptr, nullptr}, 1), MISSING);
    Views one{view(100)};
    ST(check_batch(L, BatchViewArray{one.data(), nullptr}, 0), COUNT);
    ST(batch(L, one), OK);
    // counts and items
    ST(batch(L, Views{view(0), view(1), view(256), view(257)}), OK);  // 0 + 256 + 256 + 512 items, 4 tiles
    ST(batch(L, Views(4, view(256))), OK);                            // exactly max
    ST(batch(L, Views{view(1024)}), OK);
    ST(batch(L, Views{view(0), view(0), view(1025)}), COUNT);         // (the offending view last)
    ST(batch(L, Views(3, view(257))), COUNT);                         // 1536 items, although 771 gaussians fit
    ST(batch(L, Views{view(256), view(256), view(256), view(257)}), COUNT);  // one block past max
    ST(batch(L, Views{view(1024), view(1)}), COUNT);
    ST(batch(L, Views{view(1024), view(0)}), OK);
    // dimensions
    ST(batch(L, Views{view(1), view(1, 0, 16)}), DIM);
    ST(batch(L, Views{view(1), view(1, 32, 0)}), DIM);
    ST(batch(L, Views{view(1), view(1, 65, 16)}), DIM);
    ST(batch(L, Views{view(1), view(1, 32, 33)}), DIM);
    // tiles
    ST(batch(L, Views{view(1, 64, 32)}), OK);                   // 4 tiles: the handle's
    ST(batch(L, Views{view(1, 64, 32), view(1, 1, 1)}), TILES);  // one more
    ST(batch(L, Views{view(1, 33, 16), view(1, 32, 17)}), OK);  // 2 + 2
    ST(batch(L, Views{view(1, 33, 17), view(0)}), TILES);       // 4 + 1
    ST(batch(L, Views(5, view(0))), TILES);
    const FrameLimits B = large();
    ST(batch(B, Views(65535, view(0))), OK);
    ST(batch(B, Views(65536, view(0))), TILES);
    // missing buffers
    Views v{view(1), view(1)};
    v[1].color = nullptr;
    ST(batch(L, v), MISSING);
    v = Views{view(1), view(1)};
    v[1].input.gaussians = nullptr;
    ST(batch(L, v), MISSING);
    v[1] = view(1);
    v[1].input.harmonics = nullptr;
    ST(batch(L, v), MISSING);
    v[1].input.gaussian_count = 0;  // an empty view needs no input
    v[1].input.gaussians = nullptr;
    ST(batch(L, v), OK);
    // sizes (a 32-pixel row: 256 bytes of colour, 64 of depth)
    v = Views{view(1), view(1)};
    v[1].color_pitch_bytes = 252;
    ST(batch(L, v), SIZE);
    v[1].color_pitch_bytes = 258;
    ST(batch(L, v), SIZE);
    v[1].color_pitch_bytes = 256;
    ST(batch(L, v), OK);
    v[1].color = P(0x1002);
    ST(batch(L, v), SIZE);
    v[1] = view(1);
    v[1].depth_pitch_bytes = 62;
    ST(batch(L, v), SIZE);
    v[1].depth_pitch_bytes = 65;
    ST(batch(L, v), SIZE);
    v[1].depth_pitch_bytes = 64;
    v[1].depth = P(0x2001);
    ST(batch(L, v), SIZE);
    v[1].depth = nullptr;
    v[1].depth_pitch_bytes = 1;
    ST(batch(L, v), OK);
    // sh_components
    v = Views{view(1), view(1), view(1)};
    v[2].input.sh_components = 4;
    ST(batch(L, v), ARG);
    ST(batch(restricted(), one), UNSUP);
    // options: pick and occluder join the size row where given (pixels null: not given, whatever the pitch)
    v = Views{view(1), view(1)};
    std::vector<BatchViewOptions> o(2);
    ST(batch(L, v, &o), OK);
    o[1].pick = PickTarget{nullptr, 3};
    o[1].occluder = OccluderSource{nullptr, 3};
    ST(batch(L, v, &o), OK);
    o[1].pick = PickTarget{P(0x3000), 128};
    ST(batch(L, v, &o), OK);
    o[1].pick = PickTarget{P(0x3000), 124};
    ST(batch(L, v, &o), SIZE);
    o[1].pick = PickTarget{P(0x3000), 130};
    ST(batch(L, v, &o), SIZE);
    o[1].pick = PickTarget{P(0x3002), 128};
    ST(batch(L, v, &o), SIZE);
    o[1] = BatchViewOptions{};
    o[1].occluder = OccluderSource{P(0x4000), 124};
    ST(batch(L, v, &o), SIZE);
    o[1].occluder = OccluderSource{P(0x4001), 128};
    ST(batch(L, v, &o), SIZE);
    o[1].occluder = OccluderSource{P(0x4004), 132};
    ST(batch(L, v, &o), OK);
    // the styled row per view
    o = std::vector<BatchViewOptions>(2);
    o[1].styled = true;
    o[1].style = StyleSource{kState, kStyles, 3};
    ST(batch(L, v, &o), OK);
    ST(batch(restricted(), v, &o), UNSUP);
    o[1].style.styleCount = 0;
    ST(batch(L, v, &o), ARG);
    o[1].style.styleCount = 257;
    ST(batch(L, v, &o), ARG);
    o[1].style = StyleSource{nullptr, kStyles, 3};  // styles without states
    ST(batch(L, v, &o), ARG);
    o[1].style = StyleSource{kState, nullptr, 3};   // states without styles
    ST(batch(L, v, &o), ARG);
    gsm_global_state s256{nullptr, 256, 0};
    o[1].style = StyleSource{&s256, kStyles, 3};
    ST(batch(L, v, &o), ARG);
    // one table a batch: two styled views agree in the six meaningful bytes of every style
    gsm_global_style a[3] = {{1, 2, 3, 4, 5, 0, {0, 0}}, {6, 7, 8, 9, 10, 1, {0, 0}}, {11, 12, 13, 14, 15, 0, {0, 0}}};
    gsm_global_style b[3] = {{1, 2, 3, 4, 5, 0, {9, 9}}, {6, 7, 8, 9, 10, 1, {0, 7}}, {11, 12, 13, 14, 15, 0, {7, 0}}};
    o[0].styled = o[1].styled = true;
    o[0].style = StyleSource{kState, a, 3};
    o[1].style = StyleSource{kState + 1, b, 3};
    ST(batch(L, v, &o), OK);  // (they differ in pad alone)
    o[1].style.styleCount = 2;
    ST(batch(L, v, &o), ARG);
    o[1].style.styleCount = 3;
    o[0].style.styleCount = 2;
    ST(batch(L, v, &o), ARG);
    o[0].style.styleCount = 3;
    for (int byte = 0; byte < 6; ++byte) {  // each meaningful byte of the last style
        gsm_global_style c[3] = {b[0], b[1], b[2]};
        ((uint8_t*)&c[2])[byte] ^= 1u;
        o[1].style.styles = c;
        ST(batch(L, v, &o), ARG);
    }
    o[1].style.styles = b;
    ST(batch(L, v, &o), OK);
    // two rows at once, the later one in the earlier view
    v = Views{view(1, 0, 16), view(1025)};
    ST(batch(L, v), COUNT);  // count, dimensions
    v = Views{view(1, 65, 16), view(257), view(257), view(257)};
    ST(batch(L, v), COUNT);  // items, dimensions
    v = Views(5, view(0));
    v[4].width = 65;
    ST(batch(L, v), DIM);    // dimensions, tiles
    v = Views(5, view(0));
    v[0].color = nullptr;
    ST(batch(L, v), TILES);  // tiles, missing buffer
    v = Views{view(1), view(1)};
    v[0].color_pitch_bytes = 252;
    v[1].color = nullptr;
    ST(batch(L, v), MISSING);  // missing buffer, size
    v = Views{view(1), view(1)};
    v[0].input.sh_components = 4;
    v[1].depth_pitch_bytes = 63;
    ST(batch(L, v), SIZE);  // size, sh_components
    v = Views{view(1), view(1)};
    o = std::vector<BatchViewOptions>(2);
    o[0].styled = true;
    o[0].style = StyleSource{kState, kStyles, 0};
    ST(batch(restricted(), v, &o), ARG);  // style, tile rows
    v[1].input.sh_components = 4;
    ST(batch(restricted(), v), ARG);      // sh_components, tile rows
}

static std::deque<gsm_global_object> kObjects;  // (a deque: the frames keep pointers into it)
static gsm_global_frame frame(uint32_t count, uint32_t w = 32, uint32_t h = 16) {
    gsm_global_frame F{};
    kObjects.push_back(gsm_global_object{});
    kObjects.back().input = scene(count);
    F.objects = &kObjects.back();
    F.object_count = 1;
    F.width = w;
    F.height = h;
    F.color = P(0x1000);
    F.color_pitch_bytes = 512;
    F.depth_r16f = P(0x2000);
    F.depth_pitch_bytes = 128;
    return F;
}
static gsm_status frames(const FrameLimits& L, const std::vector<gsm_global_frame>& f) {
    const gsm_status st = check_frames_front(f.data(), (uint32_t)f.size());
    return st != GSM_OK ? st : check_batch(L, BatchFrameArray{f.data()}, (uint32_t)f.size());
}

static void test_frames() {
    const FrameLimits L = small();
    using Frames = std::vector<gsm_global_frame>;
    ST(check_frames_front(nullptr, 1), MISSING);
    ST(check_frames_front(nullptr, 0), OK);
    ST(check_batch(L, BatchFrameArray{nullptr}, 0), COUNT);  // (frame_count 0: the batch's first row)
    ST(frames(L, Frames(4, frame(256))), OK);
    Frames f(3, frame(1));
    f[2].flags = GSM_FRAME_ORTHOGRAPHIC;
    ST(frames(L, f), OK);
    f[2].flags = 1;
    ST(frames(L, f), ARG);
    f[2].flags = GSM_FRAME_ORTHOGRAPHIC | 4u;
    ST(frames(L, f), ARG);
    f[2].flags = 0x80000000u;
    ST(frames(L, f), ARG);
    f[2].flags = 0;
    f[2].object_count = 0;
    ST(frames(L, f), UNSUP);
    f[2].object_count = 2;
    ST(frames(L, f), UNSUP);
    f[2].object_count = 1;
    f[2].objects = nullptr;
    ST(frames(L, f), MISSING);
    // two rows at once, the later one in the earlier frame
    f = Frames(2, frame(1));
    f[0].object_count = 2;
    f[1].flags = 1;
    ST(frames(L, f), ARG);    // flags, object_count
    f = Frames(2, frame(1));
    f[0].objects = nullptr;
    f[1].object_count = 2;
    ST(frames(L, f), UNSUP);  // object_count, objects
    f = Frames{frame(1025), frame(1)};
    f[1].objects = nullptr;
    ST(frames(L, f), MISSING);  // objects, the batch's count row
    // the batch's rows read from the frames: options
    f = Frames(2, frame(1));
    f[1].pick_r32u = P(0x3000);
    f[1].pick_pitch_bytes = 124;
    ST(frames(L, f), SIZE);
    f[1].pick_pitch_bytes = 128;
    ST(frames(L, f), OK);
    f[1].occluder_r32f = P(0x4002);
    f[1].occluder_pitch_bytes = 128;
    ST(frames(L, f), SIZE);
    f[1].occluder_r32f = P(0x4000);
    ST(frames(L, f), OK);
    f[1].states = kState;  // states without styles
    ST(frames(L, f), ARG);
    f[1].styles = kStyles;
    f[1].style_count = 256;
    ST(frames(L, f), OK);
    f[1].states = nullptr;  // styles without states
    ST(frames(L, f), ARG);
    f[1].styles = nullptr;  // neither: style_count is not read
    ST(frames(L, f), OK);
    f[1].depth_r16f = nullptr;
    f[1].depth_pitch_bytes = 1;
    ST(frames(L, f), OK);
    ST(frames(restricted(), f), UNSUP);
    // more frames than the handle's tile space holds: the count row, then the dimension row, then the tile row
    ST(frames(L, Frames(5, frame(0))), TILES);
    ST(frames(L, Frames(5, frame(1))), COUNT);  // 1280 items
    f = Frames(5, frame(0));
    f[4] = frame(1025);
    ST(frames(L, f), COUNT);
    f = Frames(5, frame(0));
    f[4].width = 65;
    ST(frames(L, f), DIM);
    f[4] = frame(1025);
    f[4].width = 65;
    ST(frames(L, f), COUNT);
    f = Frames(5, frame(0));
    f[0].color = nullptr;
    f[1].color_pitch_bytes = 3;
    ST(frames(L, f), TILES);
    ST(frames(large(), Frames(65535, frame(0))), OK);
    ST(frames(large(), Frames(65536, frame(0))), TILES);
    // what a frame's view reads
    gsm_global_frame F = frame(7, 33, 17);
    F.pick_r32u = P(0x3000);
    F.pick_pitch_bytes = 136;
    F.occluder_r32f = P(0x4000);
    F.occluder_pitch_bytes = 140;
    F.states = kState;
    F.styles = kStyles;
    F.style_count = 9;
    F.flags = GSM_FRAME_ORTHOGRAPHIC;
    const BatchViewDesc d = BatchFrameArray{&F}.at(0);
    CHECK(d.input.gaussian_count == 7 && d.input.gaussians == P(0x10000) && d.width == 33 && d.height == 17);
    CHECK(d.targets.color == P(0x1000) && d.targets.colorPitch == 512 && d.targets.depth == P(0x2000) && d.targets.depthPitch == 128);
    CHECK(d.options.pick.pixels == P(0x3000) && d.options.pick.pitch == 136 && d.options.occluder.pixels == P(0x4000) &&
          d.options.occluder.pitch == 140);
    CHECK(d.options.styled && d.options.style.states == kState && d.options.style.styles == kStyles &&
          d.options.style.styleCount == 9 && d.options.orthographic);
    F = frame(7);
    const BatchViewDesc p = BatchFrameArray{&F}.at(0);
    CHECK(!p.options.pick.pixels && !p.options.occluder.pixels && !p.options.styled && !p.options.orthographic);
}

static void test_batch_layout() {
    // counts {0, 1, 256, 257} on sizes {1x1, 32x16, 33x17, 64x32}
    const uint32_t counts[4] = {0, 1, 256, 257}, w[4] = {1, 32, 33, 64}, h[4] = {1, 16, 17, 32};
    const uint32_t blockBase[4] = {0, 0, 1, 2}, tileBase[4] = {0, 1, 2, 6}, tx[4] = {1, 1, 2, 2}, ty[4] = {1, 1, 2, 2};
    const uint32_t itemBase[4] = {0, 0, 256, 512};
    std::vector<gsm_global_view> v;
    for (int i = 0; i < 4; ++i) v.push_back(view(counts[i], w[i], h[i]));
    BatchLayout lay;
    const BatchViewArray arr{v.data(), nullptr};
    for (uint32_t i = 0; i < 4; ++i) {
        const BatchViewLayout l = lay.place(arr.at(i));
        CHECK(l.blockBase == blockBase[i] && l.tileBase == tileBase[i] && l.tilesX == tx[i] && l.tilesY == ty[i]);
        CHECK(l.itemBase == itemBase[i] && l.vec == 1 && l.align == 0);
    }
    CHECK(lay.views == 4 && lay.blocks == 4 && lay.tiles == 10 && lay.countSum == 514);
    CHECK(!lay.anyPick && !lay.anyOccluder && !lay.anyOrtho && lay.tableView == 0xFFFFFFFFu);
    // the other order: the bases follow the views before
    BatchLayout rev;
    const uint32_t rBlock[4] = {0, 2, 3, 4}, rTile[4] = {0, 4, 8, 9};
    for (uint32_t i = 0; i < 4; ++i) {
        const BatchViewLayout l = rev.place(arr.at(3 - i));
        CHECK(l.blockBase == rBlock[i] && l.tileBase == rTile[i] && l.itemBase == rBlock[i] * 256);
    }
    CHECK(rev.blocks == 4 && rev.tiles == 10 && rev.countSum == 514);
    // the wide bit: colour and its pitch at 16 bytes, depth (where there is one) and its pitch at 8
    struct Wide {
        uintptr_t color;
        size_t colorPitch;
        uintptr_t depth;
        size_t depthPitch;
        uint32_t vec;
    } const wide[] = {
        {0x1000, 512, 0, 0, 1},      {0x1010, 528, 0, 0, 1},      {0x1008, 512, 0, 0, 0},      {0x1004, 512, 0, 0, 0},
        {0x1000, 520, 0, 0, 0},      {0x1000, 516, 0, 0, 0},      {0x1000, 512, 0, 2, 1},      {0x1000, 512, 0x2000, 128, 1},
        {0x1000, 512, 0x2008, 136, 1}, {0x1000, 512, 0x2004, 128, 0}, {0x1000, 512, 0x2002, 128, 0}, {0x1000, 512, 0x2000, 132, 0},
        {0x1000, 512, 0x2000, 130, 0}, {0x1008, 512, 0x2000, 128, 0},
    };
    for (const Wide& c : wide) {
        gsm_global_view one = view(1);
        one.color = P(c.color);
        one.color_pitch_bytes = c.colorPitch;
        one.depth = P(c.depth);
        one.depth_pitch_bytes = c.depthPitch;
        BatchLayout l;
        ++checks;
        const uint32_t got = l.place(BatchViewArray{&one, nullptr}.at(0)).vec;
        if (got != c.vec) {
            ++failures;
            std::printf("FAILED wide: colour %#zx/%zu depth %#zx/%zu -> %u, expected %u\n", (size_t)c.color, c.colorPitch,
                        (size_t)c.depth, c.depthPitch, got, c.vec);
        }
    }
    // kBlendPick8 (8192) and kBlendOcc8 (16384): pixels and pitch at 8 bytes
    struct Align {
        uintptr_t pick;
        size_t pickPitch;
        uintptr_t occ;
        size_t occPitch;
        uint32_t align;
    } const align[] = {
        {0, 0, 0, 0, 0},          {0, 8, 0, 8, 0},           {0x3000, 256, 0, 0, 8192},   {0x3008, 264, 0, 0, 8192},
        {0x3004, 256, 0, 0, 0},   {0x3000, 260, 0, 0, 0},    {0, 0, 0x4000, 256, 16384},  {0, 0, 0x4004, 256, 0},
        {0, 0, 0x4000, 260, 0},   {0x3000, 256, 0x4000, 256, 24576}, {0x3004, 256, 0x4000, 256, 16384},
        {0x3000, 256, 0x4000, 252, 8192},
    };
    for (const Align& c : align) {
        gsm_global_view one = view(1);
        BatchViewOptions o;
        o.pick = PickTarget{P(c.pick), c.pickPitch};
        o.occluder = OccluderSource{P(c.occ), c.occPitch};
        BatchLayout l;
        ++checks;
        const uint32_t got = l.place(BatchViewArray{&one, &o}.at(0)).align;
        if (got != c.align) {
            ++failures;
            std::printf("FAILED align: pick %#zx/%zu occluder %#zx/%zu -> %u, expected %u\n", (size_t)c.pick, c.pickPitch,
                        (size_t)c.occ, c.occPitch, got, c.align);
        }
        CHECK(l.anyPick == (c.pick != 0) && l.anyOccluder == (c.occ != 0));
    }
    // the unions, and the first styled view's table
    std::vector<BatchViewOptions> o(4);
    o[1].orthographic = true;
    o[2].styled = true;
    o[2].style = StyleSource{kState, kStyles, 3};
    o[3].styled = true;
    o[3].style = StyleSource{kState, kStyles, 3};
    o[3].occluder = OccluderSource{P(0x4000), 256};
    BatchLayout u;
    const BatchViewArray withOptions{v.data(), o.data()};
    u.place(withOptions.at(0));
    CHECK(!u.anyPick && !u.anyOccluder && !u.anyOrtho && u.tableView == 0xFFFFFFFFu);
    u.place(withOptions.at(1));
    CHECK(!u.anyPick && !u.anyOccluder && u.anyOrtho && u.tableView == 0xFFFFFFFFu);
    u.place(withOptions.at(2));
    CHECK(!u.anyPick && !u.anyOccluder && u.anyOrtho && u.tableView == 2);
    u.place(withOptions.at(3));
    CHECK(!u.anyPick && u.anyOccluder && u.anyOrtho && u.tableView == 2);
    o[0].pick = PickTarget{P(0x3000), 256};
    o[0].styled = true;
    BatchLayout u2;
    u2.place(withOptions.at(0));
    CHECK(u2.anyPick && !u2.anyOccluder && !u2.anyOrtho && u2.tableView == 0);
}

static gsm_global_object object(uint32_t count, uint32_t sh = 1) {
    gsm_global_object O{};
    O.input = scene(count, sh);
    return O;
}

static void test_compose() {
    const FrameLimits L = small();
    using Objects = std::vector<gsm_global_object>;
    const FrameTargets t = targets();
    const FrameExtras none;
    auto compose = [&](const FrameLimits& lim, const Objects& o, const FrameTargets& tg, const FrameExtras& e, uint32_t w = 64,
                       uint32_t h = 32) { return check_compose(lim, o.data(), (uint32_t)o.size(), w, h, tg, e); };
    ST(check_compose(L, nullptr, 0, 64, 32, t, none), COUNT);
    ST(check_compose(L, nullptr, 1, 64, 32, t, none), MISSING);
    ST(check_compose(L, nullptr, 65536, 64, 32, t, none), MISSING);  // (null before the 16-bit bound)
    ST(compose(L, Objects{object(100)}, t, none), OK);
    ST(compose(L, Objects(65535, object(0)), t, none), OK);
    ST(compose(L, Objects(65536, object(0)), t, none), COUNT);
    ST(compose(L, Objects{object(0), object(1), object(256), object(257)}, t, none), OK);  // 1024 items
    ST(compose(L, Objects(4, object(256)), t, none), OK);
    ST(compose(L, Objects{object(0), object(0), object(1025)}, t, none), COUNT);  // (the offending object last)
    ST(compose(L, Objects(3, object(257)), t, none), COUNT);
    ST(compose(L, Objects{object(256), object(256), object(256), object(257)}, t, none), COUNT);
    ST(compose(L, Objects{object(1)}, t, none, 0, 32), DIM);
    ST(compose(L, Objects{object(1)}, t, none, 64, 33), DIM);
    FrameTargets bad = t;
    bad.color = nullptr;
    ST(compose(L, Objects{object(1)}, bad, none), MISSING);
    const PickTarget noPick{nullptr, 256}, pick{P(0x3000), 256};
    const OccluderSource noOcc{nullptr, 256}, occ{P(0x4000), 256};
    FrameExtras e;
    e.pick = &noPick;
    ST(compose(L, Objects{object(1)}, t, e), MISSING);
    e = none;
    e.occluder = &noOcc;
    ST(compose(L, Objects{object(1)}, t, e), MISSING);
    // a null array of a non-empty object (last); an empty object needs none
    Objects o{object(1), object(0), object(1)};
    o[1].input.gaussians = o[1].input.harmonics = nullptr;
    ST(compose(L, o, t, none), OK);
    o[2].input.harmonics = nullptr;
    ST(compose(L, o, t, none), MISSING);
    o[2] = object(1);
    o[2].input.gaussians = nullptr;
    ST(compose(L, o, t, none), MISSING);
    // sizes
    bad = t;
    bad.colorPitch = 508;
    ST(compose(L, Objects{object(1)}, bad, none), SIZE);
    bad = t;
    bad.depthPitch = 129;
    ST(compose(L, Objects{object(1)}, bad, none), SIZE);
    const PickTarget shortPick{P(0x3000), 252};
    const OccluderSource oddOcc{P(0x4002), 256};
    e = none;
    e.pick = &shortPick;
    ST(compose(L, Objects{object(1)}, t, e), SIZE);
    e = none;
    e.occluder = &oddOcc;
    ST(compose(L, Objects{object(1)}, t, e), SIZE);
    e.pick = &pick;
    e.occluder = &occ;
    ST(compose(L, Objects{object(1)}, t, e), OK);
    // sh_components
    ST(compose(L, Objects{object(1), object(0), object(1, 4)}, t, none), ARG);
    // styles: a state per object, the last one's default decides
    gsm_global_state st[3] = {{nullptr, 0, 0}, {nullptr, 255, 0}, {nullptr, 256, 0}};
    StyleSource style{st, kStyles, 256};
    e = none;
    e.style = &style;
    o = Objects{object(1), object(0), object(1)};
    ST(compose(L, o, t, e), ARG);
    st[2].default_state = 255;
    ST(compose(L, o, t, e), OK);
    style.styleCount = 257;
    ST(compose(L, o, t, e), ARG);
    style.styleCount = 0;
    ST(compose(L, o, t, e), ARG);
    style = StyleSource{nullptr, kStyles, 3};
    ST(compose(L, o, t, e), ARG);
    style = StyleSource{st, nullptr, 3};
    ST(compose(L, o, t, e), ARG);
    // tile rows: every composite is a whole frame
    ST(compose(restricted(), Objects{object(1)}, t, none), UNSUP);
    // two rows at once
    ST(compose(L, Objects{object(1025)}, t, none, 65, 32), COUNT);    // count, dimensions
    ST(compose(L, Objects(3, object(257)), t, none, 0, 32), COUNT);  // items, dimensions
    bad = t;
    bad.color = nullptr;
    ST(compose(L, Objects{object(1)}, bad, none, 65, 32), DIM);      // dimensions, missing buffer
    o = Objects{object(1), object(1)};
    o[1].input.harmonics = nullptr;
    ST(compose(L, o, t, none, 65, 32), DIM);                         // dimensions, missing input
    bad.depthPitch = 1;
    ST(compose(L, Objects{object(1)}, bad, none), MISSING);          // missing buffer, size
    o = Objects{object(1), object(1)};
    o[1].input.gaussians = nullptr;
    bad = t;
    bad.colorPitch = 508;
    ST(compose(L, o, bad, none), MISSING);                           // missing input, size
    ST(compose(L, Objects{object(1), object(1, 4)}, bad, none), SIZE);  // size, sh_components
    style = StyleSource{st, kStyles, 0};
    ST(compose(restricted(), Objects{object(1)}, t, e), ARG);        // style, tile rows
    ST(compose(restricted(), Objects{object(1), object(1, 4)}, t, none), ARG);  // sh_components, tile rows

    // the entries: empty objects first, in the middle and last take none
    const uint32_t counts[7] = {0, 0, 5, 0, 300, 256, 0};
    const bool has[7] = {false, false, true, false, true, true, false};
    const uint32_t base[7] = {0, 0, 0, 0, 1, 3, 0};
    ComposeLayout lay;
    for (uint32_t i = 0; i < 7; ++i) {
        ComposeEntry en{99, 99};
        const bool got = lay.place(counts[i], &en);
        CHECK(got == has[i]);
        if (has[i]) CHECK(en.object == i && en.blockBase == base[i]);
        else CHECK(en.object == 99 && en.blockBase == 99);
    }
    CHECK(lay.objects == 7 && lay.entries == 3 && lay.blocks == 4 && lay.countSum == 561);
    ComposeLayout two;
    ComposeEntry en{};
    CHECK(two.place(257, &en) && en.object == 0 && en.blockBase == 0);
    CHECK(two.place(1, &en) && en.object == 1 && en.blockBase == 2);
    CHECK(two.objects == 2 && two.entries == 2 && two.blocks == 3 && two.countSum == 258);
    ComposeLayout empty;
    CHECK(!empty.place(0, &en) && empty.objects == 1 && empty.entries == 0 && empty.blocks == 0 && empty.countSum == 0);
}

static void test_selects() {
    const FrameLimits L = small();
    const gsm_camera_params* cam = (const gsm_camera_params*)P(0x5000);
    const void* mask = P(0x6000);
    const uint8_t* state = (const uint8_t*)P(0x7000);
    const uint32_t* matched = (const uint32_t*)P(0x8000);
    const gsm_gaussian_input in = scene(100);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, state, nullptr, 0, matched), OK);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, state, kStyles, 256, nullptr), OK);
    ST(check_select_mask(L, nullptr, cam, 64, 32, mask, 64, state, nullptr, 0, matched), MISSING);
    gsm_gaussian_input big = scene(1025), max = scene(1024), zero = scene(0);
    ST(check_select_mask(L, &big, cam, 64, 32, mask, 64, state, nullptr, 0, matched), COUNT);
    ST(check_select_mask(L, &max, cam, 64, 32, mask, 64, state, nullptr, 0, matched), OK);
    ST(check_select_mask(L, &in, cam, 0, 32, mask, 64, state, nullptr, 0, matched), DIM);
    ST(check_select_mask(L, &in, cam, 64, 33, mask, 64, state, nullptr, 0, matched), DIM);
    ST(check_select_mask(L, &in, nullptr, 64, 32, mask, 64, state, nullptr, 0, matched), MISSING);
    ST(check_select_mask(L, &in, cam, 64, 32, nullptr, 64, state, nullptr, 0, matched), MISSING);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, nullptr, nullptr, 0, matched), MISSING);
    gsm_gaussian_input noG = in;
    noG.gaussians = nullptr;
    ST(check_select_mask(L, &noG, cam, 64, 32, mask, 64, state, nullptr, 0, matched), MISSING);
    zero.gaussians = zero.harmonics = nullptr;
    ST(check_select_mask(L, &zero, cam, 64, 32, mask, 64, nullptr, nullptr, 0, matched), OK);
    gsm_gaussian_input noH = in;  // (the select never reads harmonics)
    noH.harmonics = nullptr;
    ST(check_select_mask(L, &noH, cam, 64, 32, mask, 64, state, nullptr, 0, matched), OK);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 63, state, nullptr, 0, matched), SIZE);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 65, state, nullptr, 0, matched), OK);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, state, nullptr, 0, (const uint32_t*)P(0x8001)), SIZE);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, state, nullptr, 0, (const uint32_t*)P(0x8002)), SIZE);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, state, kStyles, 0, matched), ARG);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, state, kStyles, 257, matched), ARG);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, state, kStyles, 1, matched), OK);
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 64, state, nullptr, 3, matched), ARG);
    ST(check_select_mask(restricted(), &in, cam, 64, 32, mask, 64, state, nullptr, 0, matched), OK);  // (no tile-rows row)
    ST(check_select_mask(L, &big, cam, 65, 32, mask, 64, state, nullptr, 0, matched), COUNT);   // count, dimensions
    ST(check_select_mask(L, &in, nullptr, 65, 32, mask, 64, state, nullptr, 0, matched), DIM);  // dimensions, missing
    ST(check_select_mask(L, &in, cam, 64, 32, nullptr, 63, state, nullptr, 0, matched), MISSING);  // missing, size
    ST(check_select_mask(L, &in, cam, 64, 32, mask, 63, state, kStyles, 0, matched), SIZE);     // size, styles

    // the image rows select_pick and select_pick_ids share (a 64-pixel row of pick: 256 bytes)
    const void* pick = P(0x3000);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 256, mask, 64, state, matched), OK);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 256, nullptr, 0, state, nullptr), OK);
    ST(check_select_pick(L, 0, 64, 32, 64, 32, pick, 256, mask, 64, nullptr, matched), OK);
    ST(check_select_pick(L, 1024, 64, 32, 64, 32, pick, 256, mask, 64, state, matched), OK);
    ST(check_select_pick(L, 1025, 64, 32, 64, 32, pick, 256, mask, 64, state, matched), COUNT);
    ST(check_select_pick(L, 100, 0, 32, 0, 32, pick, 256, mask, 64, state, matched), DIM);
    ST(check_select_pick(L, 100, 65, 32, 65, 32, pick, 260, mask, 65, state, matched), DIM);
    ST(check_select_pick(L, 100, 64, 32, 32, 32, pick, 256, mask, 64, state, matched), DIM);  // not the pick frame's width
    ST(check_select_pick(L, 100, 64, 32, 64, 16, pick, 256, mask, 64, state, matched), DIM);  // nor its height
    ST(check_select_pick(L, 100, 64, 32, 64, 32, nullptr, 256, mask, 64, state, matched), MISSING);
    ST(check_select_pick(L, 1, 64, 32, 64, 32, pick, 256, mask, 64, nullptr, matched), MISSING);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 252, mask, 64, state, matched), SIZE);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 255, mask, 64, state, matched), SIZE);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 258, mask, 64, state, matched), SIZE);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 260, mask, 64, state, matched), OK);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, P(0x3001), 256, mask, 64, state, matched), SIZE);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, P(0x3002), 256, mask, 64, state, matched), SIZE);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 256, mask, 63, state, matched), SIZE);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 256, nullptr, 63, state, matched), OK);
    ST(check_select_pick(L, 100, 64, 32, 64, 32, pick, 256, mask, 64, state, (const uint32_t*)P(0x8002)), SIZE);
    ST(check_select_pick(L, 1025, 64, 32, 32, 32, pick, 256, mask, 64, state, matched), COUNT);  // count, dimensions
    ST(check_select_pick(L, 100, 64, 32, 32, 32, nullptr, 256, mask, 64, state, matched), DIM);  // dimensions, missing
    ST(check_select_pick(L, 100, 64, 32, 64, 32, nullptr, 252, mask, 64, state, matched), MISSING);  // missing, size
}

static void test_partition() {
    const FrameLimits L = small();  // two tile rows
    const uint32_t rows2[3] = {0, 1, 2}, down[3] = {0, 2, 1}, high[3] = {0, 1, 3}, flat[3] = {0, 0, 2};
    uint32_t rows16[17], rows17[18];
    for (int i = 0; i < 17; ++i) rows16[i] = i < 2 ? (uint32_t)i : 2u;
    for (int i = 0; i < 18; ++i) rows17[i] = 0;
    const void* send = P(0x9000);
    const uint32_t* counts = (const uint32_t*)P(0xA000);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, rows2, 2, true, send, counts, false), OK);
    ST(check_partition(L, scene(1000), 64, 32, 500, 500, rows2, 2, true, send, counts, false), OK);
    ST(check_partition(L, scene(1000), 64, 32, 500, 501, rows2, 2, true, send, counts, false), COUNT);
    ST(check_partition(L, scene(1), 64, 32, 0xFFFFFFFFu, 2, rows2, 2, true, send, counts, false), COUNT);  // (2^32 + 1 ids)
    ST(check_partition(L, scene(5000), 64, 32, 0, 1024, rows2, 2, true, send, counts, false), OK);
    ST(check_partition(L, scene(5000), 64, 32, 0, 1025, rows2, 2, true, send, counts, false), COUNT);
    ST(check_partition(L, scene(1000), 0, 32, 0, 1000, rows2, 2, true, send, counts, false), DIM);
    ST(check_partition(L, scene(1000), 64, 33, 0, 1000, rows2, 2, true, send, counts, false), DIM);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, nullptr, 2, true, send, counts, false), ARG);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, rows2, 0, true, send, counts, false), ARG);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, rows16, 16, true, send, counts, false), OK);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, rows17, 17, true, send, counts, false), ARG);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, rows2, 2, true, send, nullptr, false), MISSING);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, rows2, 2, true, nullptr, counts, false), MISSING);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, rows2, 2, false, nullptr, counts, false), OK);
    gsm_gaussian_input in = scene(1000);
    in.gaussians = nullptr;
    ST(check_partition(L, in, 64, 32, 0, 1000, rows2, 2, true, send, counts, false), MISSING);
    in = scene(1000);
    in.harmonics = nullptr;
    ST(check_partition(L, in, 64, 32, 0, 1000, rows2, 2, true, send, counts, false), MISSING);
    in.gaussians = nullptr;  // no ids: nothing is read
    ST(check_partition(L, in, 64, 32, 0, 0, rows2, 2, true, nullptr, counts, false), OK);
    ST(check_partition(L, in, 64, 32, 0, 0, rows2, 2, true, nullptr, nullptr, false), MISSING);
    // slab boundaries: within the handle's rows, ascending unless interleaved
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, high, 2, true, send, counts, false), ARG);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, high, 2, true, send, counts, true), ARG);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, down, 2, true, send, counts, false), ARG);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, down, 2, true, send, counts, true), OK);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, flat, 2, true, send, counts, false), OK);
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, down, 1, true, send, counts, false), OK);  // (rows past n are not read)
    // two rows at once
    ST(check_partition(L, scene(1000), 65, 32, 0, 1001, rows2, 2, true, send, counts, false), COUNT);  // count, dimensions
    ST(check_partition(L, scene(1000), 65, 32, 0, 1000, nullptr, 2, true, send, counts, false), DIM);  // dimensions, slabs
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, rows2, 17, true, send, nullptr, false), ARG);  // slabs, missing
    ST(check_partition(L, scene(1000), 64, 32, 0, 1000, high, 2, true, send, nullptr, false), MISSING);  // missing, rows
}

int main() {
    test_rules();
    test_validate_frame();
    test_single_frame();
    test_views();
    test_batch();
    test_frames();
    test_batch_layout();
    test_compose();
    test_selects();
    test_partition();
    if (failures) {
        std::printf("%d of %d checks failed\n", failures, checks);
        return 1;
    }
    std::printf("all checks passed (%d)\n", checks);
    return 0;
}
