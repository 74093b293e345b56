// TEST DOUBLE'S COMPANION (tests/test_gain_ride.py): the messages a host-only ctx keeps for nodes that no built plan holds yet
// (early_peek.h), the host's ride book, and the ride's ONE statement (fwgpu_types.h gain_ride_*, the functions the kernels compile) on
// the host, for the numpy model to be held against.  A state is a caller-owned NodeState record (128 bytes).
#include "early_peek.h"

// the host's count of frames, the frame behind which no ride is in flight (fwgpu_ctx.h RampBook, fwgpu_run.cpp note_ramps), whether the call just
// rendered could meet one, and the two parked-node figures
extern "C" void grp_ride_book(const fwgpu_ctx* c, unsigned long long* out) {
    out[0] = c->frames_done;
    out[1] = c->gain_rides.until;
    out[2] = c->gain_rides.live ? 1ull : 0ull;
    out[3] = c->gain_rides.max_n;
    out[4] = c->gain_rides.parked_n;
}
extern "C" unsigned grp_state_bytes() { return (unsigned)sizeof(fwgpu::NodeState); }
static float grp_f(unsigned bits) {
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
static unsigned grp_u(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}
// a volume (g1 = 0) or a pan at rest at (g0, g1), its smoothers settled, every other field as make_state leaves it
extern "C" void grp_init(fwgpu::NodeState* s, unsigned g0, unsigned g1) {
    memset(s, 0, sizeof(*s));
    s->sample = -1;
    s->sample_rate = 48000u;
    s->p0 = s->s0.input = s->s0.last = grp_f(g0);
    s->p1 = s->s1.input = s->s1.last = grp_f(g1);
}
// a smoother on its way: which = 0 / 1, status (SM_*), input and last as bits
extern "C" void grp_set_smoother(fwgpu::NodeState* s, int which, int status, unsigned input, unsigned last) {
    fwgpu::Smoother& m = which ? s->s1 : s->s0;
    m.status = status;
    m.input = grp_f(input);
    m.last = grp_f(last);
}
extern "C" void grp_start(fwgpu::NodeState* s, unsigned g0, unsigned g1, unsigned frames, int shape, const unsigned* ctl) {
    fwgpu::gain_ride_start(*s, grp_f(g0), grp_f(g1), frames, shape, grp_f(ctl[0]), grp_f(ctl[1]), grp_f(ctl[2]), grp_f(ctl[3]));
}
extern "C" void grp_end(fwgpu::NodeState* s) { fwgpu::gain_ride_end(*s); }
extern "C" void grp_behind_block(fwgpu::NodeState* s, unsigned frames) { fwgpu::gain_ride_behind_block(*s, frames); }
// frames j .. j + n - 1 of the block in front of the state, gain c: out = the gains' bits — the first through gain_ride_value, every
// run of four from there on through gain_ride_values<4> (what a lane of the node kernel computes): the two must agree
extern "C" int grp_frames(const fwgpu::NodeState* s, int c, unsigned j, unsigned n, unsigned* out) {
    const fwgpu::GainRide r = fwgpu::gain_ride_of(*s);
    for (unsigned i = 0; i < n; ++i) out[i] = grp_u(fwgpu::gain_ride_value(r, c, j + i));
    for (unsigned i = 0; i + 4 <= n; i += 4) {
        float g[4];
        fwgpu::gain_ride_values<4>(r, c, j + i, g);
        for (int e = 0; e < 4; ++e)
            if (grp_u(g[e]) != out[i + e]) return 0;
    }
    return 1;
}
// out = {N, k, shape, G0_0, G0_1, x1, y1, x2, y2, s0.status, s0.input, s0.last, s1.status, s1.input, s1.last, p0, p1}, floats as bits
extern "C" void grp_state(const fwgpu::NodeState* s, unsigned* out) {
    const fwgpu::GainRide r = fwgpu::gain_ride_of(*s);
    out[0] = r.N, out[1] = r.k, out[2] = (unsigned)r.shape, out[3] = grp_u(r.G0[0]), out[4] = grp_u(r.G0[1]);
    out[5] = grp_u(r.x1), out[6] = grp_u(r.y1), out[7] = grp_u(r.x2), out[8] = grp_u(r.y2);
    out[9] = (unsigned)s->s0.status, out[10] = grp_u(s->s0.input), out[11] = grp_u(s->s0.last);
    out[12] = (unsigned)s->s1.status, out[13] = grp_u(s->s1.input), out[14] = grp_u(s->s1.last);
    out[15] = grp_u(s->p0), out[16] = grp_u(s->p1);
}
// 1: the state is byte for byte grp_init(g0, g1) — what "at rest at the target" means
extern "C" int grp_is_fresh(const fwgpu::NodeState* s, unsigned g0, unsigned g1) {
    fwgpu::NodeState f;
    grp_init(&f, g0, g1);
    return memcmp(&f, s, sizeof(f)) == 0 ? 1 : 0;
}
// the curve alone, as the crossfader's xf_positions calls it: y(k / N) for n consecutive k, as bits
extern "C" void grp_curve(int shape, const unsigned* ctl, unsigned k, unsigned N, unsigned n, unsigned* out) {
    for (unsigned i = 0; i < n; ++i) {
        float u[1] = {(float)(k + i) / (float)N}, y[1];
        fwgpu::fw_curve_y<1>(shape, grp_f(ctl[0]), grp_f(ctl[1]), grp_f(ctl[2]), grp_f(ctl[3]), u, y);
        out[i] = grp_u(y[0]);
    }
}
// a message's fields back into (g0 bits, g1 bits, frames, shape, x1, y1, x2, y2)
extern "C" void grp_unpack(const unsigned* msg, unsigned* out) {
    const fwgpu::Cmd m = fwp_msg_of(msg);
    out[0] = grp_u(gr_cmd_g0(m));
    out[1] = grp_u(gr_cmd_g1(m));
    out[2] = gr_cmd_frames(m);
    out[3] = (unsigned)gr_cmd_shape(m);
    out[4] = grp_u(xf_cmd_x1(m)), out[5] = grp_u(xf_cmd_y1(m)), out[6] = grp_u(xf_cmd_x2(m)), out[7] = grp_u(xf_cmd_y2(m));
}
extern "C" void grp_pins(unsigned* out) {
    out[0] = (unsigned)fwgpu::CMD_GAIN_RIDE;
    out[1] = (unsigned)fwgpu::K_LAST;
    out[2] = (unsigned)fwgpu::K_CROSSFADE;
    out[3] = (unsigned)sizeof(fwgpu::NodeState);
    out[4] = (unsigned)sizeof(fwgpu::Cmd);
    out[5] = GAIN_RIDE_FRAMES_MAX;
}
