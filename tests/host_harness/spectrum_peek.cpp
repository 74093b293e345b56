// TEST DOUBLE'S COMPANION (tests/test_spectrum.py): the state a host-only ctx has given a node, the spectrum meter's ONE statement of
// its valid state and slice (fwgpu_types.h spec_*, the functions the plan build and the kernels compile), and floats of the ext pool
// (host memory under the fake HIP runtime) for the tables to be held against the numpy model.
#include "early_peek.h"

// the node's state as the plan build committed it (32 words), 0: no such node
extern "C" int spk_state(const fwgpu_ctx* c, long long node, unsigned* out) {
    for (uint32_t slot = 0; slot < (uint32_t)c->graph.nodes.size(); ++slot)
        if (c->graph.nodes[slot].alive && c->graph.id_of(slot) == node) {
            static_assert(sizeof(fwgpu::NodeState) == 128, "32 words");
            memcpy(out, &c->graph.nodes[slot].init, sizeof(fwgpu::NodeState));
            return 1;
        }
    return 0;
}
// out = {spec_on, spec_state_ok, win_rel, tw_rel, edges_rel, head_len, hist_rel, ring_rel, ext_len, R, N, bands, B, st.ext_off, st.ext_len}
extern "C" void spk_layout(const unsigned* st, int n_in, int n_out, unsigned* out) {
    fwgpu::NodeState s;
    memcpy(&s, st, sizeof(s));
    out[0] = fwgpu::spec_on(s) ? 1u : 0u;
    out[1] = fwgpu::spec_state_ok(s, n_in, n_out) ? 1u : 0u;
    out[2] = fwgpu::spec_win_rel(s, n_in);
    out[3] = fwgpu::spec_tw_rel(s, n_in);
    out[4] = fwgpu::spec_edges_rel(s, n_in);
    out[5] = fwgpu::spec_head_len(s);
    out[6] = fwgpu::spec_hist_rel(s, n_in);
    out[7] = fwgpu::spec_ring_rel(s, n_in);
    out[8] = fwgpu::spec_ext_len(s, n_in);
    out[9] = (unsigned)s.loop_end;
    out[10] = (unsigned)s.loop_start;
    out[11] = (unsigned)s.full_range;
    out[12] = (unsigned)s.playing;
    out[13] = s.ext_off;
    out[14] = s.ext_len;
}
// n words of the ext pool from float offset `off`; 0: past the pool's end
extern "C" int spk_ext(const fwgpu_ctx* c, unsigned off, unsigned n, unsigned* out) {
    if (!c->d_ext.p || ((size_t)off + n) * sizeof(float) > c->d_ext.cap) return 0;
    memcpy(out, (const float*)c->d_ext.p + off, (size_t)n * sizeof(float));
    return 1;
}
