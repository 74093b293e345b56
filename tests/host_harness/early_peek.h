// TEST DOUBLE'S COMPANION, the part every *_peek.cpp shares: reads the messages a host-only ctx keeps for nodes that no built plan
// holds yet (fwgpu_ctx::early_msgs — the ABI queues them there until the plan that activates the node is published), so that a test
// can see WHAT a call queued.  Header-only access: a companion is built on its own, beside the harness library, with the harness's
// include paths and flags (the layout of fwgpu_ctx is theirs; tests/fwapi.py peek_lib builds it).
#pragma once
#include <string.h>

#include "../../firewheel_amd/csrc/fwgpu_ctx.h"

extern "C" unsigned fwp_early_count(const fwgpu_ctx* c) { return c ? (unsigned)c->early_msgs.size() : 0u; }
// message i as nine 32-bit words: type, block, then the payload as it lies in the Cmd — the bits of f0, i0, i1, the low and the high
// word of d0, the low and the high word of d1; 0 = no such message
extern "C" int fwp_early_msg(const fwgpu_ctx* c, unsigned i, unsigned* out) {
    if (!c || i >= c->early_msgs.size()) return 0;
    const fwgpu::Cmd& m = c->early_msgs[i];
    static_assert(sizeof(m) == 40 && sizeof(m.state) == 4, "state, then the nine words");
    out[0] = (unsigned)m.type;
    out[1] = m.block;
    memcpy(&out[2], &m.f0, 4);
    out[3] = (unsigned)m.i0;
    out[4] = (unsigned)m.i1;
    memcpy(&out[5], &m.d0, 8);  // (little endian: the low word first)
    memcpy(&out[7], &m.d1, 8);
    return 1;
}
// ... and the nine words back into a record, for a companion that hands a message to the readers of fwgpu_types.h
static inline fwgpu::Cmd fwp_msg_of(const unsigned* w) {
    fwgpu::Cmd m{};
    m.type = (int)w[0];
    m.block = w[1];
    memcpy(&m.f0, &w[2], 4);
    m.i0 = (int)w[3];
    m.i1 = (int)w[4];
    memcpy(&m.d0, &w[5], 8);
    memcpy(&m.d1, &w[7], 8);
    return m;
}
// The layout handshake: a companion and the harness library are two builds of fwgpu_ctx.  Were their command lines ever to differ in a
// way that moves its members, early_msgs would be read from the wrong bytes without any error — so a test first asks for members
// that lie in FRONT of early_msgs (what it passed to fwgpu_ctx_create) and BEHIND it (the message vectors fwgpu_ctx_create reserves
// to exactly CMD_CAP, the drain epoch it starts at 1, the streams it has created) and goes on only if every one reads as it must.
// 0 = all as expected; else a bit per member that does not.
extern "C" int fwp_layout_check(const fwgpu_ctx* c, unsigned sample_rate, unsigned mbf, unsigned n_gin, unsigned n_gout, unsigned n_streams) {
    if (!c) return -1;
    int bad = 0;
    if (c->sample_rate != sample_rate) bad |= 1;
    if (c->mbf != mbf) bad |= 2;
    if (c->n_gin != n_gin || c->n_gout != n_gout) bad |= 4;
    if (c->cmds.capacity() != fwgpu_ctx::CMD_CAP || c->cmds.size() > c->cmds.capacity()) bad |= 8;
    if (c->drain_epoch.load(std::memory_order_relaxed) < 1 || c->drain_epoch.load(std::memory_order_relaxed) > (1ull << 40)) bad |= 16;
    if (c->early_msgs.size() > fwgpu_ctx::RING_CAP || c->early_msgs.size() > c->early_msgs.capacity()) bad |= 32;
    if (c->streams.size() != n_streams) bad |= 64;
    return bad;
}
