// TEST DOUBLE'S COMPANION (tests/test_bq_sweep.py): reads the messages a host-only ctx keeps for nodes that no built plan holds yet
// (fwgpu_ctx::early_msgs — the ABI queues them there until the plan that activates the node is published), so that a test can see
// WHAT fwgpu_biquad_sweep queued, and runs the sweep's ONE statement (fwgpu_types.h bq_sweep_*, the functions the kernels compile) on
// the host, for the numpy model to be held against.  Header-only access: built on its own, beside the harness library, with the
// harness's include paths and flags (the layout of fwgpu_ctx is theirs).
#include <string.h>

#include "../../firewheel_amd/csrc/fwgpu_ctx.h"

extern "C" unsigned bsp_early_count(const fwgpu_ctx* c) { return c ? (unsigned)c->early_msgs.size() : 0u; }
// message i: out[0] = type, out[1] = block, out[2..6] = the bits of the five coefficients as CMD_SET_COEFS packs them (f0, i0, i1, the
// low and the high word of d0), out[7], out[8] = the low and the high word of d1; 0 = no such message
extern "C" int bsp_early_msg(const fwgpu_ctx* c, unsigned i, unsigned* out) {
    if (!c || i >= c->early_msgs.size()) return 0;
    const fwgpu::Cmd& m = c->early_msgs[i];
    unsigned long long d0, d1;
    memcpy(&d0, &m.d0, 8);
    memcpy(&d1, &m.d1, 8);
    out[0] = (unsigned)m.type;
    out[1] = m.block;
    memcpy(&out[2], &m.f0, 4);
    out[3] = (unsigned)m.i0;
    out[4] = (unsigned)m.i1;
    out[5] = (unsigned)(d0 & 0xffffffffull);
    out[6] = (unsigned)(d0 >> 32);
    out[7] = (unsigned)(d1 & 0xffffffffull);
    out[8] = (unsigned)(d1 >> 32);
    return 1;
}
// the layout handshake (see sampler_fade_peek.cpp): members in FRONT of early_msgs and BEHIND it read as they must; 0 = all do
extern "C" int bsp_layout_check(const fwgpu_ctx* c, unsigned sample_rate, unsigned mbf, unsigned n_gin, unsigned n_gout) {
    if (!c) return -1;
    int bad = 0;
    if (c->sample_rate != sample_rate) bad |= 1;
    if (c->mbf != mbf) bad |= 2;
    if (c->n_gin != n_gin || c->n_gout != n_gout) bad |= 4;
    if (c->cmds.capacity() != fwgpu_ctx::CMD_CAP || c->cmds.size() > c->cmds.capacity()) bad |= 8;
    if (c->drain_epoch.load(std::memory_order_relaxed) < 1 || c->drain_epoch.load(std::memory_order_relaxed) > (1ull << 40)) bad |= 16;
    if (c->early_msgs.size() > fwgpu_ctx::RING_CAP || c->early_msgs.size() > c->early_msgs.capacity()) bad |= 32;
    return bad;
}
// the host's count of frames and of the frame behind which no sweep is in flight (fwgpu_run.cpp note_bq_sweeps)
extern "C" void bsp_sweep_book(const fwgpu_ctx* c, unsigned long long* out) {
    out[0] = c->frames_done;
    out[1] = c->bq_sweep_until;
    out[2] = c->bq_sweep_live ? 1ull : 0ull;
}

// st = {A[5], T[5] (bits), N, k}; head = the five at the head of the ext slice (bits)
static fwgpu::BqSweep bsp_load(const unsigned* st) {
    fwgpu::NodeState s;
    memset(&s, 0, sizeof(s));
    fwgpu::BqSweep w;
    memcpy(w.A, &st[0], 20);
    memcpy(w.T, &st[5], 20);
    w.N = st[10];
    w.k = st[11];
    fwgpu::bq_sweep_put(s, w);  // (through the NodeState fields the kernels keep it in)
    return fwgpu::bq_sweep_of(s);
}
static void bsp_store(const fwgpu::BqSweep& w, unsigned* st) {
    memcpy(&st[0], w.A, 20);
    memcpy(&st[5], w.T, 20);
    st[10] = w.N;
    st[11] = w.k;
}
// out[j * 5 + i] = the bits of c_i(j), j < n
extern "C" void bsp_values(const unsigned* st, const unsigned* head, unsigned n, unsigned* out) {
    const fwgpu::BqSweep w = bsp_load(st);
    for (unsigned j = 0; j < n; ++j)
        for (int i = 0; i < 5; ++i) {
            float h;
            memcpy(&h, &head[i], 4);
            const float v = fwgpu::bq_sweep_coef(w, i, j, h);
            memcpy(&out[j * 5 + (unsigned)i], &v, 4);
        }
}
// the message: 1 = the head is to be set to the target (a step)
extern "C" int bsp_start(unsigned* st, const unsigned* head, const unsigned* target, unsigned frames) {
    fwgpu::BqSweep w = bsp_load(st);
    float h[5], t[5];
    memcpy(h, head, 20);
    memcpy(t, target, 20);
    const bool step = fwgpu::bq_sweep_start(w, h, t, frames);
    bsp_store(w, st);
    return step ? 1 : 0;
}
// behind a block: 1 = the sweep is over, the head is to be set to T
extern "C" int bsp_advance(unsigned* st, unsigned frames) {
    fwgpu::BqSweep w = bsp_load(st);
    const bool over = fwgpu::bq_sweep_advance(w, frames);
    bsp_store(w, st);
    return over ? 1 : 0;
}
// a message's fields back into (five coefficient bits, frames)
extern "C" void bsp_unpack(const unsigned* msg, unsigned* out) {
    float f0;
    memcpy(&f0, &msg[2], 4);
    const unsigned long long d0 = ((unsigned long long)msg[6] << 32) | msg[5], d1 = ((unsigned long long)msg[8] << 32) | msg[7];
    double a, b;
    memcpy(&a, &d0, 8);
    memcpy(&b, &d1, 8);
    float co[5];
    fwgpu::bq_cmd_coefs(f0, (int)msg[3], (int)msg[4], a, co);
    memcpy(out, co, 20);
    out[5] = fwgpu::bq_cmd_frames(b);
}
