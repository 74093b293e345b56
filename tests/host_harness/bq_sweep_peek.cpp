// TEST DOUBLE'S COMPANION (tests/test_bq_sweep.py): the messages a host-only ctx keeps for nodes that no built plan holds yet
// (early_peek.h), the host's sweep book, and the sweep's ONE statement (fwgpu_types.h bq_sweep_*, the functions the kernels compile) on
// the host, for the numpy model to be held against.
#include "early_peek.h"

// the host's count of frames and of the frame behind which no sweep is in flight (fwgpu_ctx.h RampBook, fwgpu_run.cpp note_ramps)
extern "C" void bsp_sweep_book(const fwgpu_ctx* c, unsigned long long* out) {
    out[0] = c->frames_done;
    out[1] = c->sweeps.until;
    out[2] = c->sweeps.live ? 1ull : 0ull;
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
    const fwgpu::Cmd m = fwp_msg_of(msg);
    float co[5];
    bq_cmd_coefs(m, co);
    memcpy(out, co, 20);
    out[5] = bq_cmd_frames(m);
}
