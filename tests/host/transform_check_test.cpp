// gsm_global_transform_from_pose and the host checks of gsm_global_transform
// (gsm-renderer_amd/csrc/gsm_transform_check.h) on the CPU.  A stand-alone program over that header alone (no HIP, no
// device): the device pointers are made-up addresses that nothing dereferences.
//   transform_check_test           every refusal row of the helper and of the entry, and the order of the entry's rows
//                                  by giving two faults at once; prints "all checks passed"
//   transform_check_test poses     reads poses from the standard input, one a line -- nine rotation entries
//                                  (row-major), the scale and three translation entries, as decimal floats -- and
//                                  prints for each the status and the descriptor's 100 floats with nine digits
// tests/test_transform_ref.py builds it, once more with -fsanitize=address,undefined, and runs both.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "gsm_transform_check.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                               \
        }                                                             \
    } while (0)

static void* at(uintptr_t a) { return (void*)a; }
static const float kInf = std::numeric_limits<float>::infinity();
static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static const float kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
static const float kZero[3] = {0, 0, 0};

static void test_from_pose_rows() {
    gsm_global_transform_desc d;
    EXPECT(gsm::transform_from_pose(kIdentity, 1.0f, kZero, &d) == GSM_OK);
    // the identity gives the identity, exactly
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) EXPECT(d.matrix[4 * r + c] == (r == c ? 1.0f : 0.0f));
    EXPECT(d.quaternion[0] == 0.0f && d.quaternion[1] == 0.0f && d.quaternion[2] == 0.0f && d.quaternion[3] == 1.0f);
    EXPECT(d.scale == 1.0f);
    for (int i = 0; i < 9; ++i) EXPECT(d.sh1[i] == (i % 4 == 0 ? 1.0f : 0.0f));
    for (int i = 0; i < 25; ++i) EXPECT(d.sh2[i] == (i % 6 == 0 ? 1.0f : 0.0f));
    for (int i = 0; i < 49; ++i) EXPECT(d.sh3[i] == (i % 8 == 0 ? 1.0f : 0.0f));
    // NULL pointers
    EXPECT(gsm::transform_from_pose(nullptr, 1.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::transform_from_pose(kIdentity, 1.0f, nullptr, &d) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::transform_from_pose(kIdentity, 1.0f, kZero, nullptr) == GSM_ERR_INVALID_ARGUMENT);
    // non-finite inputs
    const float bad[3] = {kNaN, kInf, -kInf};
    for (float v : bad) {
        for (int i = 0; i < 9; ++i) {
            float R[9];
            std::memcpy(R, kIdentity, sizeof(R));
            R[i] = v;
            EXPECT(gsm::transform_from_pose(R, 1.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
        }
        for (int i = 0; i < 3; ++i) {
            float t[3] = {0, 0, 0};
            t[i] = v;
            EXPECT(gsm::transform_from_pose(kIdentity, 1.0f, t, &d) == GSM_ERR_INVALID_ARGUMENT);
        }
        EXPECT(gsm::transform_from_pose(kIdentity, v, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
    }
    // the scale
    EXPECT(gsm::transform_from_pose(kIdentity, 0.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::transform_from_pose(kIdentity, -1.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::transform_from_pose(kIdentity, 1e-30f, kZero, &d) == GSM_OK);
    // no rotation: a scale in R, a shear, a reflection; 5e-5 off is accepted, 2e-4 off is not
    const float scaled[9] = {2, 0, 0, 0, 2, 0, 0, 0, 2};
    const float shear[9] = {1, 0.01f, 0, 0, 1, 0, 0, 0, 1};
    const float mirror[9] = {1, 0, 0, 0, 1, 0, 0, 0, -1};
    const float swap[9] = {0, 1, 0, 1, 0, 0, 0, 0, 1};
    const float near_[9] = {1.00002f, 0, 0, 0, 1, 0, 0, 0, 1};
    const float far_[9] = {1.0001f, 0, 0, 0, 1, 0, 0, 0, 1};
    EXPECT(gsm::transform_from_pose(scaled, 1.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::transform_from_pose(shear, 1.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::transform_from_pose(mirror, 1.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::transform_from_pose(swap, 1.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::transform_from_pose(near_, 1.0f, kZero, &d) == GSM_OK);
    EXPECT(gsm::transform_from_pose(far_, 1.0f, kZero, &d) == GSM_ERR_INVALID_ARGUMENT);
}

struct Call {
    gsm_global_scene scene;
    gsm_global_state st;
    uint32_t keep[8];
    gsm_global_transform_desc desc;
    uint32_t maxGaussians;
    bool half;
    gsm_status run() const { return gsm::transform_check(maxGaussians, half, &scene, &st, keep, &desc); }
};

// 1000 gaussians of 16 components, every pointer given, the identity
static Call good(bool half) {
    Call c;
    std::memset(&c, 0, sizeof(c));
    c.scene.gaussians = at(0x100000);
    c.scene.harmonics = at(0x400000);
    c.scene.gaussian_count = 1000;
    c.scene.sh_components = 16;
    c.st.state = (const uint8_t*)at(0x300003);  // (a state array has no alignment)
    for (int k = 0; k < 8; ++k) c.keep[k] = 0xFFFFFFFFu;
    gsm::transform_from_pose(kIdentity, 1.0f, kZero, &c.desc);
    c.maxGaussians = 1000;
    c.half = half;
    return c;
}

static void test_check_rows(bool half) {
    Call c = good(half);
    EXPECT(c.run() == GSM_OK);
    c.scene.gaussian_count = 1001;
    EXPECT(c.run() == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    // scene, state, keep, desc
    c = good(half);
    EXPECT(gsm::transform_check(1000, half, nullptr, &c.st, c.keep, &c.desc) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::transform_check(1000, half, &c.scene, nullptr, c.keep, &c.desc) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::transform_check(1000, half, &c.scene, &c.st, nullptr, &c.desc) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::transform_check(1000, half, &c.scene, &c.st, c.keep, nullptr) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    // gaussians with a count; harmonics with a count and more than one component
    c = good(half); c.scene.gaussians = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(half); c.scene.harmonics = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    for (uint32_t sh = 0; sh < 2; ++sh) {
        c = good(half); c.scene.harmonics = nullptr; c.scene.sh_components = sh;
        EXPECT(c.run() == GSM_OK);
        c = good(half); c.scene.harmonics = at(0x400001); c.scene.sh_components = sh;  // (not read: any address)
        EXPECT(c.run() == GSM_OK);
    }
    c = good(half); c.scene.gaussians = nullptr; c.scene.harmonics = nullptr; c.scene.gaussian_count = 0;
    EXPECT(c.run() == GSM_OK);
    c = good(half); c.st.state = nullptr; c.st.default_state = 255;  // ({NULL, s}: every gaussian's state)
    EXPECT(c.run() == GSM_OK);
    // alignment: the records 16 bytes; the harmonics their element, and 16 bytes for the fp16 row of 16
    for (uintptr_t off = 1; off < 16; ++off) {
        c = good(half); c.scene.gaussians = at(0x100000 + off);
        EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    }
    const uint32_t comps[3] = {4, 9, 16};
    for (uint32_t sh : comps)
        for (uintptr_t off = 1; off < 16; ++off) {
            c = good(half); c.scene.sh_components = sh; c.scene.harmonics = at(0x400000 + off);
            const uintptr_t need = half ? (sh == 16 ? 16 : 2) : 4;
            EXPECT(c.run() == (off % need ? GSM_ERR_INVALID_BUFFER_SIZE : GSM_OK));
            EXPECT(gsm::transform_wide_rows(half, sh, c.scene.harmonics) == false);
        }
    EXPECT(gsm::transform_wide_rows(half, 4, at(0x400000)) == !half);   // 48 B rows; 24 B rows
    EXPECT(gsm::transform_wide_rows(half, 9, at(0x400000)) == false);   // 108 B; 54 B
    EXPECT(gsm::transform_wide_rows(half, 16, at(0x400000)) == true);   // 192 B; 96 B
    // the arguments
    c = good(half); c.st.default_state = 256;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    const uint32_t wrong[6] = {2, 3, 5, 15, 17, 25};
    for (uint32_t sh : wrong) {
        c = good(half); c.scene.sh_components = sh;
        EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    }
    const float bad[3] = {kNaN, kInf, -kInf};
    float* const f = reinterpret_cast<float*>(&c.desc);
    for (int i = 0; i < 100; ++i)
        for (float v : bad) {
            c = good(half); f[i] = v;
            EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
        }
    c = good(half); c.desc.scale = 0.0f;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(half); c.desc.scale = -2.0f;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(half); c.desc.sh3[5] = 7.0f; c.desc.quaternion[0] = 3.0f;  // (applied as given: no rotation, not refused)
    EXPECT(c.run() == GSM_OK);
    // the byte ranges: 1000 records of 48 or 32 bytes from 0x100000; the rows just past them are fine
    const uintptr_t rec = half ? 32 : 48;
    c = good(half); c.scene.harmonics = at(0x100000 + 1000 * rec);
    EXPECT(c.run() == GSM_OK);
    c = good(half); c.scene.harmonics = at(0x100000 + 1000 * rec - 16);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(half); c.scene.harmonics = at(0x100000);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(half); c.scene.gaussians = at(0x400000 + 1000 * 48 * (half ? 2 : 4) - 16);  // the last row's last bytes
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(half); c.scene.gaussians = at(0x400000 + 1000 * 48 * (half ? 2 : 4));
    EXPECT(c.run() == GSM_OK);
    c = good(half); c.scene.harmonics = at(0x100000); c.scene.sh_components = 1;  // (not read: may meet)
    EXPECT(c.run() == GSM_OK);
}

static void test_check_order(bool half) {
    // two faults at once: the earlier row decides
    Call c = good(half);
    c.scene.gaussian_count = 1001;
    EXPECT(gsm::transform_check(1000, half, &c.scene, nullptr, c.keep, &c.desc) == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    c = good(half); c.scene.gaussian_count = 1001; c.scene.gaussians = nullptr;
    EXPECT(c.run() == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    c = good(half); c.scene.gaussians = at(0x100004);
    EXPECT(gsm::transform_check(1000, half, &c.scene, &c.st, c.keep, nullptr) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(half); c.scene.harmonics = nullptr; c.scene.gaussians = at(0x100004);
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(half); c.scene.gaussians = at(0x100004); c.st.default_state = 256;
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(half); c.scene.harmonics = at(0x400001); c.desc.scale = 0.0f;
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(half); c.scene.harmonics = at(0x400001); c.scene.sh_components = 5;
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
}

static int print_poses() {
    float v[13];
    for (;;) {
        for (int i = 0; i < 13; ++i)
            if (std::scanf("%f", &v[i]) != 1) return 0;
        gsm_global_transform_desc d;
        std::memset(&d, 0, sizeof(d));
        const gsm_status st = gsm::transform_from_pose(v, v[9], v + 10, &d);
        std::printf("%d", (int)st);
        const float* f = reinterpret_cast<const float*>(&d);
        for (int i = 0; i < 100; ++i) std::printf(" %.9g", (double)f[i]);
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "poses") == 0) return print_poses();
    test_from_pose_rows();
    for (int half = 0; half < 2; ++half) {
        test_check_rows(half != 0);
        test_check_order(half != 0);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
