// TEST DOUBLE'S COMPANION (tests/test_fir_morph.py): the messages a host-only ctx holds back (early_peek.h), the host's bookkeeping of a
// morph-capable FirReverbNode, the FIR groups of the active plan image, and the morph's ONE statement (fwgpu_types.h fir_morph_*, the
// functions the kernels compile) on the host, for the numpy model to be held against.  A state is a caller-owned NodeState (128 bytes).
#include "early_peek.h"

static float fmp_f(unsigned bits) {
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
static unsigned fmp_u(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}
extern "C" unsigned fmp_state_bytes() { return (unsigned)sizeof(fwgpu::NodeState); }
// a morph-capable node of one channel as activation leaves it: at rest at `position`, T taps, a ring of R, one block record behind it
extern "C" void fmp_init(fwgpu::NodeState* s, unsigned position, int law, unsigned T, unsigned R) {
    memset(s, 0, sizeof(*s));
    s->sample = 0;
    s->sample_rate = 48000u;
    s->enabled = 1;
    s->p0 = s->p1 = fmp_f(position);
    s->playing = law;
    s->loop_start = T;
    s->loop_end = R;
    s->ext_off = 64;
    s->ext_len = (uint32_t)fwgpu::fir_morph_ext_len(R, 1, 1);
    s->s1.input = fwgpu::fw_float_of(64u + fwgpu::fir_morph_tab_rel(R, 1));
    s->s1.last = fwgpu::fw_float_of(1u);
}
extern "C" int fmp_state_ok(const fwgpu::NodeState* s, int n_in, int n_out) { return fwgpu::fir_morph_state_ok(*s, n_in, n_out) ? 1 : 0; }
extern "C" void fmp_msg(fwgpu::NodeState* s, unsigned position, unsigned frames, int shape, const unsigned* ctl) {
    fwgpu::fir_morph_msg(*s, fmp_f(position), frames, shape, fmp_f(ctl[0]), fmp_f(ctl[1]), fmp_f(ctl[2]), fmp_f(ctl[3]));
}
// one block: the record (16 words) the control step leaves, the state advanced; returns the block's mode
extern "C" int fmp_block(fwgpu::NodeState* s, unsigned frames, unsigned* rec) {
    const fwgpu::FirMorphBlk b = fwgpu::fir_morph_block(*s, frames);
    memcpy(rec, &b, sizeof(b));
    return b.mode;
}
// frames 0 .. n-1 of the block whose record is `rec`, from the two slot sums (as bits) -> the output's bits
extern "C" void fmp_out(const unsigned* rec, unsigned n, const unsigned* sa, const unsigned* sb, unsigned* out) {
    fwgpu::FirMorphBlk b;
    memcpy(&b, rec, sizeof(b));
    const fwgpu::XfSeg g = fwgpu::fir_morph_seg(b);
    const unsigned long long T0 = (unsigned long long)b.T_lo | ((unsigned long long)b.T_hi << 32);
    for (unsigned i = 0; i < n; ++i) out[i] = fmp_u(fwgpu::fir_morph_out(b, g, T0 + i, fmp_f(sa[i]), fmp_f(sb[i])));
}
// node time and t0 of a state
extern "C" void fmp_times(const fwgpu::NodeState* s, unsigned long long* out) {
    out[0] = fwgpu::fir_morph_time(*s);
    out[1] = fwgpu::fir_morph_t0(*s);
}
// the host's bookkeeping of a node: {fir_morph, ir_a, ir_b, max_taps, target bits, hold, activated, T, R, ext_off, ext_len, enabled,
// block records' offset, block records, morphs held}; and the end of the last morph
extern "C" int fmp_node(fwgpu_ctx* c, long long node, long long* out, unsigned long long* target_end) {
    const unsigned slot = (unsigned)(node & 0xffffffff);  // (header-only access: the id is generation << 32 | slot)
    if (slot >= c->graph.nodes.size()) return 0;
    const fwgpu::HostNode* n = &c->graph.nodes[slot];
    if (!n->alive || n->gen != (unsigned)(node >> 32)) return 0;
    out[0] = n->fir_morph ? 1 : 0, out[1] = n->fir_ir[0], out[2] = n->fir_ir[1], out[3] = n->fir_max_taps, out[4] = fmp_u(n->fir_target);
    out[5] = n->fir_hold ? 1 : 0, out[6] = n->activated ? 1 : 0, out[7] = (long long)n->init.loop_start, out[8] = (long long)n->init.loop_end;
    out[9] = n->init.ext_off, out[10] = n->init.ext_len, out[11] = n->init.enabled;
    out[12] = fwgpu::fir_morph_tab(n->init), out[13] = fwgpu::fir_morph_tab_n(n->init), out[14] = n->fir_held;
    *target_end = n->fir_target_end;
    return 1;
}
// the ctx: {frames_done, frames_ctl, converted copies cached, ext floats in use, entries in limbo, ext slices on the free lists}
extern "C" void fmp_ctx(const fwgpu_ctx* c, unsigned long long* out) {
    out[0] = c->frames_done;
    out[1] = c->frames_ctl.load();
    out[2] = c->ir_cache.size();
    out[3] = c->ext_used;
    out[4] = c->limbo.size();
    unsigned long long n = 0;
    for (const auto& kv : c->ext_free) n += kv.second.size();
    out[5] = n;
}
// converted copy i of the cache: {sample, channel, padded length, ext offset}; 0 = no such entry
extern "C" int fmp_cached(const fwgpu_ctx* c, unsigned i, long long* out) {
    if (i >= c->ir_cache.size()) return 0;
    auto it = c->ir_cache.begin();
    std::advance(it, i);
    out[0] = std::get<0>(it->first), out[1] = std::get<1>(it->first), out[2] = std::get<2>(it->first), out[3] = it->second;
    return 1;
}
// FIR group i of the ACTIVE plan image: {level, T, morph, rows, A rows, B rows, padding rows}; 0 = no such group.  (The harness's
// device memory is host memory: the row table is read in place.)
extern "C" int fmp_group(const fwgpu_ctx* c, unsigned i, long long* out) {
    if (i >= c->fir_groups.size()) return 0;
    const fwgpu_ctx::FirGroup& g = c->fir_groups[i];
    out[0] = g.level, out[1] = g.T, out[2] = g.morph, out[3] = g.n_rows;
    long long a = 0, b = 0, pad = 0;
    const fwgpu::FirRow* rows = c->d_fir_rows.as<fwgpu::FirRow>() + g.row_off;
    for (int r = 0; r < g.n_rows; ++r) {
        if (rows[r].state < 0) pad++;
        else if (rows[r].in_buf < 0) b++;
        else a++;
    }
    out[4] = a, out[5] = b, out[6] = pad;
    return 1;
}
// the partner table of morph group i holds: every A row's partner is a B row of the same state and channel (or none), and back; every
// tile has rows of one slot kind only where they share an impulse response.  1 = consistent
extern "C" int fmp_group_partners_ok(const fwgpu_ctx* c, unsigned i) {
    if (i >= c->fir_groups.size()) return 0;
    const fwgpu_ctx::FirGroup& g = c->fir_groups[i];
    if (!g.morph) return 1;
    const fwgpu::FirRow* rows = c->d_fir_rows.as<fwgpu::FirRow>() + g.row_off;
    const uint32_t* partner = c->d_fir_tiles.as<uint32_t>() + g.tile_off + g.n_rows / 32;
    for (int r = 0; r < g.n_rows; ++r) {
        if (rows[r].state < 0) {
            if (partner[r] != FIR_NO_PARTNER) return 0;
            continue;
        }
        const uint32_t q = partner[r];
        if (q == FIR_NO_PARTNER) {
            if (rows[r].in_buf < 0) return 0;  // a B row always has its A row
            continue;
        }
        if (q >= (uint32_t)g.n_rows || partner[q] != (uint32_t)r) return 0;
        if (rows[q].state != rows[r].state || rows[q].ch != rows[r].ch || (rows[q].in_buf < 0) == (rows[r].in_buf < 0)) return 0;
        if (rows[q].out_buf != rows[r].out_buf) return 0;
    }
    return 1;
}
extern "C" void fmp_pins(unsigned* out) {
    out[0] = (unsigned)fwgpu::CMD_XF_TO;
    out[1] = (unsigned)fwgpu::K_FIR;
    out[2] = (unsigned)sizeof(fwgpu::NodeState);
    out[3] = (unsigned)sizeof(fwgpu::FirRow);
    out[4] = (unsigned)sizeof(fwgpu::FirMorphBlk);
    out[5] = (unsigned)sizeof(fwgpu::DevView);
    out[6] = FIR_SEG;
}
