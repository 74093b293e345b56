// TEST DOUBLE'S COMPANION (tests/test_rs_glide.py): reads the messages a host-only ctx keeps for nodes that no built plan holds yet
// (fwgpu_ctx::early_msgs — the ABI queues them there until the plan that activates the node is published), so that a test can see
// WHAT a call queued: the Cmd's type, block, i0 and the bits of d0.  Header-only access: built on its own, beside the harness library,
// with the harness's include paths and flags (the layout of fwgpu_ctx is theirs).
#include <string.h>

#include "../../firewheel_amd/csrc/fwgpu_ctx.h"

extern "C" unsigned rsg_early_count(const fwgpu_ctx* c) { return c ? (unsigned)c->early_msgs.size() : 0u; }
// message i: out[0] = type, out[1] = block, out[2] = i0, out[3] / out[4] = the low / high 32 bits of d0; 0 = no such message
extern "C" int rsg_early_msg(const fwgpu_ctx* c, unsigned i, unsigned* out) {
    if (!c || i >= c->early_msgs.size()) return 0;
    const fwgpu::Cmd& m = c->early_msgs[i];
    unsigned long long u;
    memcpy(&u, &m.d0, 8);
    out[0] = (unsigned)m.type;
    out[1] = m.block;
    out[2] = (unsigned)m.i0;
    out[3] = (unsigned)(u & 0xffffffffull);
    out[4] = (unsigned)(u >> 32);
    return 1;
}
// The layout handshake: this file and the harness library are two builds of fwgpu_ctx.  Were their command lines ever to differ in a
// way that moves its members, early_msgs would be read from the wrong bytes without any error — so the test first asks for members
// that lie in FRONT of early_msgs (what it passed to fwgpu_ctx_create) and BEHIND it (the message vectors fwgpu_ctx_create reserves
// to exactly CMD_CAP, the drain epoch it starts at 1) and goes on only if every one reads as it must.  0 = all as expected; else a
// bit per member that does not.
extern "C" int rsg_layout_check(const fwgpu_ctx* c, unsigned sample_rate, unsigned mbf, unsigned n_gin, unsigned n_gout) {
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
