// TEST DRIVER, CPU tier only (tests/test_stream_source.py builds it with -fsanitize=address,undefined against the host-only harness
// — fake HIP runtime + launch stubs, no audio computed — and runs it as a child process).  It plays a host application that feeds
// streaming sample sources (SPEC) over a seeded schedule of writes, process calls, pauses and ends, and holds the control
// side's accounting to a shadow of its own:
//   - a write accepts exactly min(frames, R - (written - consumed as last published)) frames, and never more than the true free space;
//   - every frame in [C, written) reads back from the ring as it was written (nothing unread is ever overwritten), in the split at the
//     ring's end and per channel for the planar formats;
//   - fwgpu_sample_stream_status reports the counts of the last process call, `finished` behind the end and not before;
//   - a full message ring leaves `written` where it was and the repeated call succeeds; writes behind `end` are refused.
// The launch stubs render nothing, so the driver plays the sampler itself: before each process call it moves the sampler's NodeState in
// the fake device memory with the functions the kernels compile (fwgpu_types.h smp_stream_*); the call then publishes that state.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/fwgpu.h"
#include "../../firewheel_amd/csrc/fwgpu_ctx.h"

#define CHECK(x)                                                                      \
    do {                                                                              \
        if (!(x)) {                                                                   \
            fprintf(stderr, "stream_driver: CHECK failed: %s (line %d)\n", #x, __LINE__); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

static uint64_t rng_state = 1;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static size_t elem_size(int fmt) { return (fmt == FWGPU_INTERLEAVED_F32 || fmt == FWGPU_PLANAR_F32) ? 4 : 2; }
// element (frame, ch) of the shadow: a value that names its place
static uint32_t shadow_elem(uint64_t frame, int ch, size_t es) {
    const uint32_t v = (uint32_t)(frame * 7u + (uint64_t)ch * 3u + 1u);
    return es == 2 ? (v & 0xffffu) : v;
}

static void run(int fmt, int channels, uint32_t mbf, uint64_t R, int steps) {
    fwgpu_ctx* c = fwgpu_ctx_create(0, 48000, mbf, 0, 2, nullptr);
    CHECK(c);
    float pv = 100.f;
    const int64_t smp = fwgpu_add_node(c, FWGPU_SAMPLER, 0, 2, &pv, 1);
    CHECK(smp >= 0);
    CHECK(fwgpu_connect(c, smp, 0, fwgpu_graph_out_node(c), 0, 0) >= 0);
    CHECK(fwgpu_connect(c, smp, 1, fwgpu_graph_out_node(c), 1, 0) >= 0);
    CHECK(fwgpu_update(c) == 0);
    const int id = fwgpu_sample_create_stream(c, fmt, (uint32_t)channels, R);
    CHECK(id >= 0);
    const size_t es = elem_size(fmt);
    const bool planar = fmt >= FWGPU_PLANAR_I16;
    const int slot = (int)(smp & 0xffffffff);
    std::vector<float> out(2 * (size_t)mbf * 4);
    uint64_t written = 0, pub_C = 0, pub_U = 0;  // the shadow: frames accepted; C and U as the last process call published them
    bool bound = false, ended = false, pub_finished = false;
    uint64_t end_at = 0;
    auto state = [&]() -> NodeState& { return c->d_states.as<NodeState>()[slot]; };
    auto process = [&](uint32_t blocks) {
        if (bound) {  // the device's part, played here: the call's messages (W, E), then its blocks
            NodeState& s = state();
            smp_stream_msg(s, written + (ended ? mbf : 0), ended ? 1 : 0, end_at);
            for (uint32_t b = 0; b < blocks; ++b) {
                if (!s.playing || smp_stream_starved(s, mbf)) continue;
                const uint64_t ph0 = s.playhead;
                s.playhead = (s.playhead >= s.loop_end ? 0 : s.playhead) + mbf;
                if (s.playhead > s.loop_end) s.playhead -= s.loop_end;
                smp_stream_behind_block(s, ph0, mbf);
            }
        }
        CHECK(fwgpu_process_interleaved(c, nullptr, out.data(), 0, 2, (uint64_t)blocks * mbf, 0.0, 0) == 0);
        if (bound) {
            const SmpStream t = smp_stream_of(state());
            pub_C = t.C, pub_U = t.U, pub_finished = (t.flags & SMP_STREAM_FINISHED) != 0;
        }
    };
    auto check_ring = [&]() {  // every unread frame is where it was put
        const uint64_t C = bound ? smp_stream_of(state()).C : 0;
        const unsigned char* ring = (const unsigned char*)c->samples[id].desc.data;
        for (uint64_t f = C; f < written; ++f)
            for (int k = 0; k < channels; ++k) {
                const uint64_t pos = f % R, at = planar ? (uint64_t)k * R + pos : pos * (uint64_t)channels + (uint64_t)k;
                uint32_t got = 0;
                memcpy(&got, ring + at * es, es);
                CHECK(got == shadow_elem(f, k, es));
            }
    };
    auto check_status = [&]() {
        uint64_t w = 0, cc = 0, u = 0;
        int fin = -1;
        CHECK(fwgpu_sample_stream_status(c, id, &w, &cc, &u, &fin) == 0);
        CHECK(w == written && cc == pub_C && u == pub_U && fin == (pub_finished ? 1 : 0));
    };
    std::vector<unsigned char> buf;
    for (int step = 0; step < steps; ++step) {
        const uint32_t what = rnd() % 16;
        if (!bound && (what == 0 || step == steps / 8)) {
            CHECK(fwgpu_sampler_set_sample(c, smp, id, 0, 0) == 0);
            CHECK(fwgpu_sampler_set_sample(c, smp, id, 0, 0) == FWGPU_ERR_INVALID);  // bound once
            CHECK(fwgpu_sampler_play(c, smp, 0) == 0);
            NodeState& s = state();
            s.sample = id;
            smp_stream_bind(s, R, written);
            s.playing = 1;
            bound = true;
        } else if (what < 9 && !ended) {  // a write of 0 .. 2.5 blocks, sometimes far more than fits
            const uint64_t frames = what == 1 ? R + rnd() % 100 : rnd() % (5 * mbf / 2 + 1);
            buf.assign((size_t)(frames ? frames : 1) * channels * es, 0);
            for (uint64_t f = 0; f < frames; ++f)
                for (int k = 0; k < channels; ++k) {
                    const uint32_t v = shadow_elem(written + f, k, es);
                    const uint64_t at = planar ? (uint64_t)k * frames + f : f * (uint64_t)channels + (uint64_t)k;
                    memcpy(&buf[at * es], &v, es);
                }
            const uint64_t free_seen = R - (written - pub_C), want = frames < free_seen ? frames : free_seen;
            int rc = fwgpu_sample_stream_write(c, id, buf.data(), frames);
            if (rc == FWGPU_ERR_QUEUE_FULL) {  // `written` has not moved; a process call drains the ring and the same call succeeds
                check_status();
                process(1);
                const uint64_t free2 = R - (written - pub_C);
                rc = fwgpu_sample_stream_write(c, id, buf.data(), frames);
                CHECK(rc == (int)(frames < free2 ? frames : free2));
            } else {
                CHECK(rc == (int)want);
            }
            CHECK(rc >= 0 && (uint64_t)rc <= R - (written - (bound ? smp_stream_of(state()).C : 0)));  // never more than is truly free
            written += (uint64_t)rc;
            check_ring();
        } else if (what < 13) {
            process(1 + rnd() % 3);
        } else if (what == 13 && bound) {
            const bool pause = state().playing != 0;
            CHECK((pause ? fwgpu_sampler_pause(c, smp, 0) : fwgpu_sampler_play(c, smp, 0)) == 0);
            if (pause) smp_pause(state());
            else if (!smp_stream_finished(state())) state().playing = 1;
        } else if (what == 14 && !ended && step > steps / 2) {
            const uint64_t free_seen = R - (written - pub_C);
            const int rc = fwgpu_sample_stream_end(c, id);
            if (free_seen < mbf) {
                CHECK(rc == FWGPU_ERR_QUEUE_FULL);
            } else if (rc == FWGPU_ERR_QUEUE_FULL) {  // (the sampler's message ring)
                process(1);
            } else {
                CHECK(rc == 0);
                ended = true;
                end_at = written;
                CHECK(fwgpu_sample_stream_write(c, id, buf.data(), 1) == FWGPU_ERR_INVALID);
                CHECK(fwgpu_sample_stream_end(c, id) == FWGPU_ERR_INVALID);
            }
        }
        check_status();
    }
    if (bound && !ended) {
        while (fwgpu_sample_stream_end(c, id) != 0) process(1);
        ended = true;
        end_at = written;
    }
    if (bound) {
        if (!state().playing && !smp_stream_finished(state())) {
            CHECK(fwgpu_sampler_play(c, smp, 0) == 0);
            state().playing = 1;
        }
        for (int i = 0; i < 64 && !pub_finished; ++i) process(3);
        CHECK(pub_finished && pub_C >= end_at && pub_C < end_at + mbf);
        check_status();
        uint64_t w, cc, u;
        int fin;
        CHECK(fwgpu_sample_stream_status(c, id, &w, &cc, &u, &fin) == 0 && fin == 1);
        CHECK(c->stream_pub_n == 0);  // a finished stream is no longer published
    }
    CHECK(fwgpu_sample_destroy(c, id) == 0);
    fwgpu_ctx_destroy(c);
}

int main(int argc, char** argv) {
    const int seeds = argc > 1 ? atoi(argv[1]) : 6;
    for (int seed = 1; seed <= seeds; ++seed) {
        rng_state = (uint64_t)seed * 0x9e3779b97f4a7c15ull;
        run(FWGPU_INTERLEAVED_I16, 2, 64, 4 * 64 + 24, 400);
        run(FWGPU_PLANAR_F32, 2, 64, 6 * 64, 400);
        run(FWGPU_PLANAR_U16, 1, 32, 4 * 32 + 5, 300);
        run(FWGPU_INTERLEAVED_F32, 3, 64, 9 * 64 + 1, 300);
    }
    printf("stream-driver ok: %d seeds\n", seeds);
    return 0;
}
