// TEST DOUBLE'S COMPANION (tests/test_sampler_fade.py): reads the messages a host-only ctx keeps for nodes that no built plan holds yet
// (fwgpu_ctx::early_msgs — the ABI queues them there until the plan that activates the node is published), so that a test can see
// WHAT a call queued: the Cmd's type, block, i0, the bits of f0 and i1.  Header-only access: built on its own, beside the harness
// library, with the harness's include paths and flags (the layout of fwgpu_ctx is theirs).
#include <string.h>

#include "../../firewheel_amd/csrc/fwgpu_ctx.h"

extern "C" unsigned sfp_early_count(const fwgpu_ctx* c) { return c ? (unsigned)c->early_msgs.size() : 0u; }
// message i: out[0] = type, out[1] = block, out[2] = i0, out[3] = the bits of f0, out[4] = i1; 0 = no such message
extern "C" int sfp_early_msg(const fwgpu_ctx* c, unsigned i, unsigned* out) {
    if (!c || i >= c->early_msgs.size()) return 0;
    const fwgpu::Cmd& m = c->early_msgs[i];
    unsigned f;
    memcpy(&f, &m.f0, 4);
    out[0] = (unsigned)m.type;
    out[1] = m.block;
    out[2] = (unsigned)m.i0;
    out[3] = f;
    out[4] = (unsigned)m.i1;
    return 1;
}
// The layout handshake: this file and the harness library are two builds of fwgpu_ctx.  Were their command lines ever to differ in a
// way that moves its members, early_msgs would be read from the wrong bytes without any error — so the test first asks for members
// that lie in FRONT of early_msgs (what it passed to fwgpu_ctx_create) and BEHIND it (the message vectors fwgpu_ctx_create reserves
// to exactly CMD_CAP, the drain epoch it starts at 1) and goes on only if every one reads as it must.  0 = all as expected; else a
// bit per member that does not.
extern "C" int sfp_layout_check(const fwgpu_ctx* c, unsigned sample_rate, unsigned mbf, unsigned n_gin, unsigned n_gout) {
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
// The envelope's ONE statement (fwgpu_types.h smp_env_*, the functions the kernels compile) on the host, for the model to be held
// against: st = {bits of E0 (phasor), bits of E1 (gain), enabled (N and `then`), s1.status (k), playing, has_loop, playhead, loop_start}
static fwgpu::NodeState sfp_load(const unsigned* st) {
    fwgpu::NodeState s;
    memset(&s, 0, sizeof(s));
    memcpy(&s.phasor, &st[0], 4);
    memcpy(&s.gain, &st[1], 4);
    s.enabled = (int)st[2];
    s.s1.status = (int)st[3];
    s.playing = (int)st[4];
    s.has_loop = (int)st[5];
    s.playhead = st[6];
    s.loop_start = st[7];
    return s;
}
static void sfp_store(const fwgpu::NodeState& s, unsigned* st) {
    memcpy(&st[0], &s.phasor, 4);
    memcpy(&st[1], &s.gain, 4);
    st[2] = (unsigned)s.enabled;
    st[3] = (unsigned)s.s1.status;
    st[4] = (unsigned)s.playing;
    st[5] = (unsigned)s.has_loop;
    st[6] = (unsigned)s.playhead;
    st[7] = (unsigned)s.loop_start;
}
extern "C" void sfp_env_values(const unsigned* st, unsigned n, unsigned* out_bits) {
    const fwgpu::SmpEnv e = fwgpu::smp_env_of(sfp_load(st));
    for (unsigned j = 0; j < n; ++j) {
        const float v = fwgpu::smp_env_value(e, j);
        memcpy(&out_bits[j], &v, 4);
    }
}
extern "C" void sfp_env_start(unsigned* st, unsigned target_bits, unsigned frames, int then) {
    fwgpu::NodeState s = sfp_load(st);
    float t;
    memcpy(&t, &target_bits, 4);
    fwgpu::smp_env_start(s, t, frames, then);
    sfp_store(s, st);
}
extern "C" void sfp_env_behind_block(unsigned* st, unsigned frames) {
    fwgpu::NodeState s = sfp_load(st);
    fwgpu::smp_env_behind_block(s, frames);
    sfp_store(s, st);
}
