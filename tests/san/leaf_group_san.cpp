// Stand-alone sanitizer run of the HOST code of grouped calls: this program, the library's host translation units and
// the host-only harness (tests/host_harness: fake HIP runtime, launch stubs) built into one executable with
// -fsanitize=address,undefined — scripts/run_leaf_group_san.sh builds and runs it.  CPU only: no device code is involved, nothing is
// loaded into an interpreter.  It builds an eligible bank (12 voices, 3 leaf mixers, a root), runs 2 control calls and 20 lazy calls
// of 8 blocks with the switch on, and checks that exactly the 20 lazy batches were grouped and that the launch stubs saw no violation.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/fwgpu.h"

extern "C" const char* fwh_violation(void);

#define CHECK(x)                                                             \
    do {                                                                     \
        if (!(x)) {                                                          \
            fprintf(stderr, "leaf_group_san: %s failed (line %d)\n", #x, __LINE__); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

int main() {
    setenv("FWGPU_LEAF_GROUP", "1", 1);
    setenv("FWGPU_LEAF_GROUP_MIN", "1", 1);
    const uint32_t mbf = 64, K = 8;
    fwgpu_ctx* c = fwgpu_ctx_create(0, 48000, mbf, 0, 2, nullptr);
    CHECK(c != nullptr);
    CHECK(fwgpu_set_max_batch(c, K) == 0);
    std::vector<int64_t> samplers, leaves;
    for (int l = 0; l < 3; ++l) {
        const int64_t leaf = fwgpu_add_node(c, FWGPU_SUM, 8, 2, nullptr, 0);
        CHECK(leaf >= 0);
        for (int p = 0; p < 4; ++p) {
            const float sv = 90.0f, vv = 50.0f + (float)(4 * l + p), pv = 0.1f * (float)p - 0.2f;
            const int64_t s = fwgpu_add_node(c, FWGPU_SAMPLER, 0, 2, &sv, 1);
            const int64_t v = fwgpu_add_node(c, FWGPU_VOLUME, 2, 2, &vv, 1);
            const int64_t q = fwgpu_add_node(c, FWGPU_STEREO_PAN, 2, 2, &pv, 1);
            CHECK(s >= 0 && v >= 0 && q >= 0);
            for (uint32_t ch = 0; ch < 2; ++ch) {
                CHECK(fwgpu_connect(c, s, ch, v, ch, 0) >= 0);
                CHECK(fwgpu_connect(c, v, ch, q, ch, 0) >= 0);
                CHECK(fwgpu_connect(c, q, ch, leaf, 2 * p + ch, 0) >= 0);
            }
            samplers.push_back(s);
        }
        leaves.push_back(leaf);
    }
    const int64_t root = fwgpu_add_node(c, FWGPU_SUM, 6, 2, nullptr, 0);
    CHECK(root >= 0);
    for (uint32_t l = 0; l < 3; ++l)
        for (uint32_t ch = 0; ch < 2; ++ch) CHECK(fwgpu_connect(c, leaves[l], ch, root, 2 * l + ch, 0) >= 0);
    for (uint32_t ch = 0; ch < 2; ++ch) CHECK(fwgpu_connect(c, root, ch, fwgpu_graph_out_node(c), ch, 0) >= 0);
    CHECK(fwgpu_update(c) == 0);
    CHECK(fwgpu_plan_kind(c) == 1);
    std::vector<float> data(2 * 4 * mbf, 0.25f);
    for (int64_t s : samplers) {
        const int smp = fwgpu_sample_create(c, FWGPU_PLANAR_F32, 2, 4 * mbf, data.data());
        CHECK(smp >= 0);
        CHECK(fwgpu_sampler_set_sample(c, s, smp, 0, 0) == 0);
        CHECK(fwgpu_sampler_set_loop_range(c, s, 1, 0.0, 0.0, 0) == 0);
        CHECK(fwgpu_sampler_play(c, s, 0) == 0);
    }
    std::vector<float> out((size_t)K * mbf * 2);
    for (int call = 0; call < 22; ++call) CHECK(fwgpu_process_interleaved(c, nullptr, out.data(), 0, 2, (uint64_t)K * mbf, 0.0, 0) == 0);
    uint64_t grouped = 0, lazy = 0, ctl = 0;
    CHECK(fwgpu_plan_group_stats(c, &grouped) == 0 && fwgpu_lazy_stats(c, &lazy, &ctl) == 0);
    printf("leaf_group_san: %llu grouped of %llu lazy batches, %llu control batches, violation '%s'\n", (unsigned long long)grouped,
           (unsigned long long)lazy, (unsigned long long)ctl, fwh_violation());
    CHECK(grouped == 20 && lazy == 20 && ctl == 2);
    CHECK(fwh_violation()[0] == 0);
    fwgpu_ctx_destroy(c);
    printf("leaf_group_san ok\n");
    return 0;
}
