// TEST DOUBLE'S COMPANION (tests/test_sampler_fade.py): the messages a host-only ctx keeps for nodes that no built plan holds yet
// (early_peek.h), and the envelope's ONE statement on the host.
#include "early_peek.h"

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
