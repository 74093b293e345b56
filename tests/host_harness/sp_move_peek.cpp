// TEST DOUBLE'S COMPANION (tests/test_sp_move.py): the messages a host-only ctx keeps for nodes that no built plan holds yet
// (early_peek.h), the host's move book, and the move's ONE statement (fwgpu_types.h sp_move_*, the functions the kernels compile) on
// the host, for the numpy model to be held against.  A state is a caller-owned NodeState record (128 bytes).
#include "early_peek.h"

// the host's count of frames and of the frame behind which no move is in flight (fwgpu_ctx.h RampBook, fwgpu_run.cpp note_ramps)
extern "C" void spp_move_book(const fwgpu_ctx* c, unsigned long long* out) {
    out[0] = c->frames_done;
    out[1] = c->moves.until;
    out[2] = c->moves.live ? 1ull : 0ull;
}
extern "C" unsigned spp_state_bytes() { return (unsigned)sizeof(fwgpu::NodeState); }
static float spp_f(unsigned bits) {
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
static unsigned spp_u(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}
// a spatialiser at rest at (gl, gr, dl, dr), its smoothers settled, every other field as make_state leaves it
extern "C" void spp_init(fwgpu::NodeState* s, unsigned gl, unsigned gr, int dl, int dr) {
    memset(s, 0, sizeof(*s));
    s->sample = -1;
    s->p0 = s->s0.input = s->s0.last = spp_f(gl);
    s->p1 = s->s1.input = s->s1.last = spp_f(gr);
    s->playing = dl;
    s->has_loop = dr;
}
// a smoother on its way: which = 0 / 1, status (SM_*), input and last as bits
extern "C" void spp_set_smoother(fwgpu::NodeState* s, int which, int status, unsigned input, unsigned last) {
    fwgpu::Smoother& m = which ? s->s1 : s->s0;
    m.status = status;
    m.input = spp_f(input);
    m.last = spp_f(last);
}
extern "C" void spp_start(fwgpu::NodeState* s, unsigned gl, unsigned gr, int dl, int dr, unsigned frames) {
    fwgpu::sp_move_start(*s, spp_f(gl), spp_f(gr), dl, dr, frames);
}
extern "C" void spp_stop(fwgpu::NodeState* s) { fwgpu::sp_move_stop(*s); }
extern "C" void spp_advance(fwgpu::NodeState* s, unsigned frames) { fwgpu::sp_move_advance(*s, frames); }
// frame j of the block in front of the state: out = {gain bits l, gain bits r, D l, D r}
extern "C" void spp_frame(const fwgpu::NodeState* s, unsigned j, unsigned long long* out) {
    const fwgpu::SpMove m = fwgpu::sp_move_of(*s);
    out[0] = spp_u(fwgpu::sp_move_gain(m, 0, j));
    out[1] = spp_u(fwgpu::sp_move_gain(m, 1, j));
    out[2] = fwgpu::sp_move_delay(m, 0, j);
    out[3] = fwgpu::sp_move_delay(m, 1, j);
}
// out = {N, k, D l, D r, inc l, inc r, playing, has_loop, s0.status, s0.input, s0.last, s1.status, s1.input, s1.last, p0, p1}
extern "C" void spp_state(const fwgpu::NodeState* s, unsigned long long* out) {
    const fwgpu::SpMove m = fwgpu::sp_move_of(*s);
    out[0] = m.N, out[1] = m.k, out[2] = m.D[0], out[3] = m.D[1], out[4] = m.inc[0], out[5] = m.inc[1];
    out[6] = (unsigned)s->playing, out[7] = (unsigned)s->has_loop;
    out[8] = (unsigned)s->s0.status, out[9] = spp_u(s->s0.input), out[10] = spp_u(s->s0.last);
    out[11] = (unsigned)s->s1.status, out[12] = spp_u(s->s1.input), out[13] = spp_u(s->s1.last);
    out[14] = spp_u(s->p0), out[15] = spp_u(s->p1);
}
// the two taps blended: a, b as bits, D the 32.32 delay; the word the voice bank's rows carry must give the same whole and fraction
extern "C" unsigned spp_tap(unsigned a, unsigned b, unsigned long long D) {
    const unsigned w = fwgpu::sp_move_word(D);
    if (fwgpu::sp_word_whole(w) != fwgpu::sp_move_whole(D) || spp_u(fwgpu::sp_word_frac(w)) != spp_u(fwgpu::sp_move_frac(D))) return 0xffffffffu;
    return spp_u(fwgpu::sp_move_tap(spp_f(a), spp_f(b), fwgpu::sp_move_frac(D)));
}
// a message's fields back into (gl bits, gr bits, dl, dr, frames)
extern "C" void spp_unpack(const unsigned* msg, unsigned* out) {
    const fwgpu::Cmd m = fwp_msg_of(msg);
    out[0] = spp_u(sp_cmd_gl(m));
    out[1] = spp_u(sp_cmd_gr(m));
    out[2] = (unsigned)sp_cmd_dl(m);
    out[3] = (unsigned)sp_cmd_dr(m);
    out[4] = sp_cmd_frames(m);
}
extern "C" void spp_pins(unsigned* out) {
    out[0] = (unsigned)fwgpu::CMD_SP_MOVE;
    out[1] = (unsigned)fwgpu::K_LAST;
    out[2] = (unsigned)fwgpu::K_CROSSFADE;
    out[3] = (unsigned)sizeof(fwgpu::NodeState);
    out[4] = (unsigned)sizeof(fwgpu::Cmd);
    out[5] = SP_MOVE_FRAMES_MAX;
}
