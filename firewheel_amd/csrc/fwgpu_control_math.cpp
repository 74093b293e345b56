// fwgpu_control_math.cpp — control-half scalar math, done on the host exactly as the reference's control thread does it,
// and the initial audio-half state of every node kind (the AudioNode constructors + activate()).
#include "fwgpu_ctx.h"

namespace fwgpu {

// ---- control-half scalar math, done on the host exactly as the reference's control thread does it
float percent_volume_to_raw_gain(float p) {  // core/param/range.rs:32-35
    float n = fmaxf(p, 0.0f) * (1.0f / 100.0f);
    return n * n;
}
float db_to_gain_clamped_neg_100_db(float db) {  // core/util.rs:7-9,21-27
    if (db <= -100.0f) return 0.0f;
    return powf(10.0f, 0.05f * db);
}
void pan_to_gains(float pan, float* gl, float* gr) {  // SPEC: DESIGN.md "spec nodes / pan"
    float p = fminf(fmaxf(pan, -1.0f), 1.0f);
    if (p <= -1.0f) {
        *gl = 1.0f;
        *gr = 0.0f;
        return;
    }
    if (p >= 1.0f) {
        *gl = 0.0f;
        *gr = 1.0f;
        return;
    }
    double theta = ((double)p + 1.0) * (3.14159265358979323846 / 4.0);
    *gl = (float)cos(theta);
    *gr = (float)sin(theta);
}
Smoother make_smoother(float val, uint32_t sample_rate) {  // core/param/smoother.rs:93-112, defaults :18-25
    Smoother s;
    const float smooth_secs = 10.0f / 1000.0f;
    s.b = expf(-1.0f / (smooth_secs * (float)sample_rate));
    s.a = 1.0f - s.b;
    s.status = SM_INACTIVE;
    s.input = val;
    s.last = val;
    s.eps = 0.00001f;
    return s;
}

// SPEC biquad: RBJ cookbook, computed in f64 on the control side, normalised by a0, rounded to f32.
void biquad_coefs(int type, float cutoff_hz, float q, uint32_t sample_rate, float co[5]) {
    double fs = (double)sample_rate;
    double f0 = fmin(fmax((double)cutoff_hz, 1.0), 0.49 * fs);
    double Q = fmax((double)q, 1e-3);
    double w0 = 2.0 * 3.14159265358979323846 * f0 / fs;
    double cw = cos(w0), alpha = sin(w0) / (2.0 * Q);
    double b0, b1, b2, a0 = 1.0 + alpha, a1 = -2.0 * cw, a2 = 1.0 - alpha;
    if (type == 1) {  // high-pass
        b0 = (1.0 + cw) * 0.5;
        b1 = -(1.0 + cw);
        b2 = (1.0 + cw) * 0.5;
    } else if (type == 2) {  // band-pass, constant 0 dB peak gain
        b0 = alpha;
        b1 = 0.0;
        b2 = -alpha;
    } else {  // low-pass
        b0 = (1.0 - cw) * 0.5;
        b1 = 1.0 - cw;
        b2 = (1.0 - cw) * 0.5;
    }
    co[0] = (float)(b0 / a0);
    co[1] = (float)(b1 / a0);
    co[2] = (float)(b2 / a0);
    co[3] = (float)(a1 / a0);
    co[4] = (float)(a2 / a0);
}
// SPEC resampler: Kaiser-windowed sinc (beta 8, cutoff 0.9 x Nyquist), RS_PHASES x RS_TAPS, every
// phase normalised to unity DC gain in f64 and rounded to f32 — the control side builds the table once per ctx.
double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; ++k) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
    }
    return sum;
}
void resampler_table(float* h) {
    const double fc = 0.9, beta = 8.0, half = RS_TAPS / 2.0, pi = 3.14159265358979323846;
    const double i0b = bessel_i0(beta);
    for (int ph = 0; ph < RS_PHASES; ++ph) {
        double row[RS_TAPS], sum = 0.0;
        for (int k = 0; k < RS_TAPS; ++k) {
            double t = (double)(k - (RS_TAPS / 2 - 1)) - (double)ph / RS_PHASES;
            double x = pi * fc * t;
            double sinc = fabs(t) < 1e-12 ? 1.0 : sin(x) / x;
            double r = t / half;
            double w = fabs(r) >= 1.0 ? 0.0 : bessel_i0(beta * sqrt(1.0 - r * r)) / i0b;
            row[k] = fc * sinc * w;
            sum += row[k];
        }
        for (int k = 0; k < RS_TAPS; ++k) h[ph * RS_TAPS + k] = (float)(row[k] / sum);
    }
}
uint64_t resampler_step(float ratio) {  // source frames per output frame as 32.32 fixed point
    double r = (double)ratio;
    if (!(r >= 1.0 / 256.0)) r = 1.0 / 256.0;
    if (r > 256.0) r = 256.0;
    return (uint64_t)llround(r * 4294967296.0);
}
// SPEC spatialiser: listener at the origin (+x right, +y up, -z forward): inverse-distance gain (reference distance
// 1, rolloff 1), equal-power pan from the direction cosine to the right, per-ear delay up to 0.66 ms.
void spatial_params(float x, float y, float z, uint32_t sample_rate, float* gl, float* gr, int* dl, int* dr) {
    const double pi = 3.14159265358979323846;
    double d = sqrt((double)x * x + (double)y * y + (double)z * z);
    double att = 1.0 / fmax(d, 1.0);
    double s = d < 1e-9 ? 0.0 : (double)x / d;
    double theta = (s + 1.0) * (pi / 4.0);
    *gl = (float)(cos(theta) * att);
    *gr = (float)(sin(theta) * att);
    double itd_max = round(0.00066 * (double)sample_rate);
    if (itd_max > SP_HIST - 1) itd_max = SP_HIST - 1;
    *dl = (int)round(fmax(0.0, s) * itd_max);
    *dr = (int)round(fmax(0.0, -s) * itd_max);
}
// SPEC compressor: the static curve in decibels, computed in f64 on the control side and rounded to f32.  T0 is the level
// at which the knee begins; knot i of the table sits at u_i = 2^(i / 16) * (1 + (i % 16) / 16) times T0 — where the top four mantissa
// bits of an f32 change — and holds the linear gain there.  G[0] is exactly 1 (gr = 0 at u = 1) and G never rises.
float compressor_knee_start(float threshold, float knee_db) { return (float)((double)threshold * pow(10.0, -(double)knee_db / 40.0)); }
void compressor_table(float ratio, float knee_db, float G[COMP_TAB_PAD]) {
    const double knee = (double)knee_db, slope = 1.0 / (double)ratio - 1.0;
    for (int i = 0; i < COMP_TAB_PAD; ++i) G[i] = 0.0f;
    for (int i = 0; i < COMP_TAB_N; ++i) {
        const double u = ldexp(1.0 + (double)(i % 16) / 16.0, i / 16);
        const double over = 20.0 * log10(u) - knee / 2.0;  // decibels above the threshold
        double gr = 0.0;
        if (knee > 0.0 && 2.0 * fabs(over) <= knee) {
            const double t = over + knee / 2.0;
            gr = slope * (t * t) / (2.0 * knee);
        } else if (over > 0.0) {
            gr = slope * over;
        }
        G[i] = (float)pow(10.0, gr / 20.0);
    }
}
// SPEC spectrum meter: the band edges e[0..B] over the bins of an N-point transform; bands == 0: every bin, DC included
void spectrum_edges(uint32_t N, uint32_t bands, uint32_t* e) {
    const int M = (int)(N / 2), B = (int)bands;
    if (B == 0) {
        for (int b = 0; b <= M + 1; ++b) e[b] = (uint32_t)b;
        return;
    }
    e[0] = 1;
    for (int b = 1; b < B; ++b) {
        const int want = (int)floor(pow((double)M, (double)b / B) + 0.5), cap = M + 1 - (B - b);
        const int lo = (int)e[b - 1] + 1, v = cap < want ? cap : want;
        e[b] = (uint32_t)(lo > v ? lo : v);
    }
    e[B] = (uint32_t)(M + 1);
}
// ... and the slice's head (fwgpu_types.h spec_head_len floats): the periodic Hann window w[N], the twiddles wr[N/2] wi[N/2], the edges
// as raw 32-bit words, zeros up to the head's length
void spectrum_tables(const NodeState& s, float* head) {
    const uint32_t N = (uint32_t)s.loop_start, B = (uint32_t)s.playing;
    for (uint32_t i = 0; i < N; ++i) head[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / N));
    for (uint32_t k = 0; k < N / 2; ++k) {
        head[N + k] = (float)cos(2.0 * M_PI * k / N);
        head[N + N / 2 + k] = (float)(-sin(2.0 * M_PI * k / N));
    }
    std::vector<uint32_t> e(B + 1);
    spectrum_edges(N, (uint32_t)s.full_range, e.data());
    for (uint32_t b = 0; b < spec_head_len(s) - 2 * N; ++b) head[2 * N + b] = fw_float_of(b <= B ? e[b] : 0u);
}
uint32_t delay_frames(float secs, uint32_t sample_rate) {
    double d = round((double)secs * (double)sample_rate);
    if (!(d >= 1.0)) d = 1.0;
    if (d > 16777216.0) d = 16777216.0;
    return (uint32_t)d;
}

// AudioNode constructors + activate(): the initial audio-half state of each node kind.
NodeState make_state(int kind, const float* params, int n_params, uint32_t sample_rate) {
    auto p = [&](int i, float d) { return i < n_params ? params[i] : d; };
    NodeState s;
    memset(&s, 0, sizeof(s));
    s.sample = -1;
    s.sample_rate = sample_rate;
    s.s0 = make_smoother(0.f, sample_rate);
    s.s1 = make_smoother(0.f, sample_rate);
    switch (kind) {
        case K_VOLUME:   // volume.rs:15-22, :67-75
        case K_SAMPLER:  // sampler.rs:55-64, :302-319
            s.p0 = percent_volume_to_raw_gain(fmaxf(p(0, 100.0f), 0.0f));
            s.s0 = make_smoother(s.p0, sample_rate);
            if (kind == K_SAMPLER) smp_env_reset(s);  // SPEC gain envelope: a new sampler rests at 1.0f
            break;
        case K_BEEP: {  // beep_test.rs:15-24, :55-60
            float f = p(0, 440.0f);
            if (f < 20.0f) f = 20.0f;
            if (f > 20000.0f) f = 20000.0f;
            float g = db_to_gain_clamped_neg_100_db(p(1, -12.0f));
            if (g < 0.0f) g = 0.0f;
            if (g > 1.0f) g = 1.0f;
            s.gain = g;
            s.enabled = p(2, 1.0f) != 0.0f ? 1 : 0;
            s.phasor = 0.0f;
            s.phasor_inc = f / (float)sample_rate;
            break;
        }
        case K_HARD_CLIP:  // hard_clip.rs:8-12
            s.p0 = db_to_gain_clamped_neg_100_db(p(0, 0.0f));
            break;
        case K_PAN:
            pan_to_gains(p(0, 0.0f), &s.p0, &s.p1);
            s.s0 = make_smoother(s.p0, sample_rate);
            s.s1 = make_smoother(s.p1, sample_rate);
            break;
        case K_WIDTH:
            s.p0 = fmaxf(p(0, 1.0f), 0.0f);
            s.s0 = make_smoother(s.p0, sample_rate);
            break;
        case K_BIQUAD:  // coefficients go to the ext pool at activation; keep the ctor args for that
            s.p0 = p(1, 1000.0f);  // cutoff
            s.p1 = p(2, 0.70710678f);  // Q
            s.enabled = (int)p(0, 0.0f);  // type
            break;
        case K_FIR:
            s.sample = (int)p(0, -1.0f);  // impulse-response sample id; T and the ring are set at activation
            if (n_params >= 2) {  // SPEC FIR morph (fwgpu_types.h fir_morph_*): ir_a, ir_b, max_taps, position, law
                const float irb = p(1, -1.0f), taps = p(2, 0.0f), pos = p(3, 0.0f), law = p(4, (float)XF_LAW_EQUAL_POWER);
                // anything else — NaN, out of range, a fraction, another law — sets s0.status, and the node fails activation at the next update
                const bool ok = irb >= -1.0f && irb <= 16777216.0f && irb == floorf(irb) && taps >= 0.0f && taps <= 16777216.0f && taps == floorf(taps) &&
                                pos >= 0.0f && pos <= 1.0f && (law == (float)XF_LAW_LINEAR || law == (float)XF_LAW_EQUAL_POWER);
                memset(&s.s0, 0, sizeof(s.s0));  // node time 0, t0 0
                memset(&s.s1, 0, sizeof(s.s1));
                s.enabled = 1;
                s.s0.status = ok ? 0 : 1;
                s.s1.status = ok ? (int)irb : -1;                   // (the host's bookkeeping takes these two over: HostNode::fir_ir, fir_max_taps)
                s.s1.a = fw_float_of(ok ? (uint32_t)taps : 0u);
                s.p0 = s.p1 = ok ? pos : 0.0f;  // at rest at `position`: dur (full_range) 0
                s.playing = ok ? (int)law : XF_LAW_EQUAL_POWER;
                s.has_loop = XF_SHAPE_LINEAR;
            }
            break;
        case K_RESAMPLER:  // params: sample id, ratio, loop, playing
            s.sample = (int)p(0, -1.0f);
            s.loop_start = resampler_step(p(1, 1.0f));
            s.has_loop = p(2, 0.0f) != 0.0f ? 1 : 0;
            s.playing = p(3, 1.0f) != 0.0f ? 1 : 0;
            s.playhead = 0;
            break;
        case K_SPATIAL: {  // params: x, y, z of the source; the ctor args stay in phasor / phasor_inc / gain
            s.phasor = p(0, 0.0f);
            s.phasor_inc = p(1, 0.0f);
            s.gain = p(2, -1.0f);
            int dl, dr;
            spatial_params(s.phasor, s.phasor_inc, s.gain, sample_rate, &s.p0, &s.p1, &dl, &dr);
            s.s0 = make_smoother(s.p0, sample_rate);
            s.s1 = make_smoother(s.p1, sample_rate);
            s.playing = dl;
            s.has_loop = dr;
            break;
        }
        case K_DELAY: {
            float mix = fminf(fmaxf(p(2, 0.5f), 0.0f), 1.0f);
            s.p0 = fminf(fmaxf(p(1, 0.0f), 0.0f), 0.999f);  // feedback
            s.p1 = mix;
            s.gain = 1.0f - mix;  // dry
            s.loop_end = delay_frames(p(0, 0.1f), sample_rate);
            s.playhead = 0;
            break;
        }
        case K_METER: {  // params: ring_blocks (how many blocks of readings the node retains), 1..65536, default 1024
            const float r = p(0, (float)METER_RING_DEFAULT);
            // anything else — NaN, a fraction, out of range — leaves 0 here, and the node fails activation at the next update
            s.loop_end = (r >= 1.0f && r <= (float)METER_RING_MAX && r == floorf(r)) ? (uint64_t)r : 0;
            if (n_params >= 2) {  // SPEC spectrum meter (fwgpu_types.h spec_*): ring_blocks, fft_size, bands
                const float n = p(1, 0.0f), b = p(2, (float)SPEC_BANDS_DEFAULT);
                const bool pow2 = n == 256.0f || n == 512.0f || n == 1024.0f || n == 2048.0f || n == 4096.0f;
                if (s.loop_end != 0 && pow2 && b >= 0.0f && b <= n / 2.0f && b == floorf(b)) {
                    s.loop_start = (uint64_t)n;
                    s.full_range = (int)b;
                    s.playing = b == 0.0f ? (int)n / 2 + 1 : (int)b;
                } else {  // (loop_start says whose message the refusal gets)
                    s.loop_end = 0;
                    s.loop_start = 1;
                }
            }
            break;
        }
        case K_LIMITER: {  // params: ceiling (linear, 0.001..1000, default 1.0), hold_frames (0..1920, default 128)
            const float ceil_ = p(0, 1.0f), h = p(1, (float)LIM_HOLD_DEFAULT);
            // anything else — NaN, inf, a fraction, out of range — leaves loop_end 0, and the node fails activation at the next update
            const bool ok = ceil_ >= 0.001f && ceil_ <= 1000.0f && h >= 0.0f && h <= (float)LIM_HOLD_MAX && h == floorf(h);
            s.p0 = ok ? ceil_ : 1.0f;
            s.loop_start = ok ? (uint64_t)h : 0;
            s.loop_end = ok ? (uint64_t)h + LIM_HIST_PAD : 0;
            break;
        }
        case K_DUCKER: {  // params: threshold (linear, 1e-6..1000), depth (0..1), attack_frames, release_frames (1..32768), hold_frames (0..32768)
            const float t = p(0, DUCK_THRESHOLD_DEFAULT), d = p(1, DUCK_DEPTH_DEFAULT), a = p(2, (float)DUCK_ATTACK_DEFAULT),
                        r = p(3, (float)DUCK_RELEASE_DEFAULT), h = p(4, (float)DUCK_HOLD_DEFAULT);
            // anything else — NaN, inf, a fraction, out of range — leaves loop_end 0, and the node fails activation at the next update
            const bool ok = t >= 1e-6f && t <= 1000.0f && d >= 0.0f && d <= 1.0f && a >= 1.0f && a <= (float)DUCK_WIN_MAX && a == floorf(a) &&
                            r >= 1.0f && r <= (float)DUCK_WIN_MAX && r == floorf(r) && h >= 0.0f && h <= (float)DUCK_HOLD_MAX && h == floorf(h);
            s.p0 = ok ? t : DUCK_THRESHOLD_DEFAULT;
            s.p1 = ok ? d : 1.0f;
            s.playhead = ok ? (uint64_t)a : 1;
            s.loop_start = ok ? (uint64_t)r : 1;
            s.full_range = ok ? (int)h : 0;
            s.loop_end = ok ? (uint64_t)(a > r ? a : r) + (uint64_t)h : 0;
            break;
        }
        case K_COMPRESSOR: {  // params: threshold (linear, 1e-6..1000), ratio (1..1000), knee_db (0..24), attack_frames, release_frames
                              // (1..32768), hold_frames (0..2048), makeup (linear, 0.001..1000)
            const float t = p(0, COMP_THRESHOLD_DEFAULT), ratio = p(1, COMP_RATIO_DEFAULT), knee = p(2, COMP_KNEE_DEFAULT),
                        a = p(3, (float)COMP_ATTACK_DEFAULT), r = p(4, (float)COMP_RELEASE_DEFAULT), h = p(5, (float)COMP_HOLD_DEFAULT),
                        m = p(6, COMP_MAKEUP_DEFAULT);
            // anything else — NaN, inf, a fraction, out of range — leaves loop_end 0, and the node fails activation at the next update
            const bool ok = t >= 1e-6f && t <= 1000.0f && ratio >= 1.0f && ratio <= 1000.0f && knee >= 0.0f && knee <= 24.0f && a >= 1.0f &&
                            a <= (float)COMP_WIN_MAX && a == floorf(a) && r >= 1.0f && r <= (float)COMP_WIN_MAX && r == floorf(r) && h >= 0.0f &&
                            h <= (float)COMP_HOLD_MAX && h == floorf(h) && m >= 0.001f && m <= 1000.0f;
            s.phasor_inc = ok ? t : COMP_THRESHOLD_DEFAULT;
            s.gain = ok ? ratio : 1.0f;
            s.phasor = ok ? knee : 0.0f;
            s.p0 = compressor_knee_start(s.phasor_inc, s.phasor);
            s.p1 = ok ? m : 1.0f;
            s.playhead = ok ? (uint64_t)a : 1;
            s.loop_start = ok ? (uint64_t)r : 1;
            s.full_range = ok ? (int)h : 0;
            s.loop_end = ok ? (uint64_t)(a > r ? a : r) + (uint64_t)h : 0;
            break;
        }
        case K_DELAY_COMP: {  // params: frames (the delay D, a whole number in 0..8192, default 63)
            const float d = p(0, (float)DCOMP_DEFAULT);
            // anything else — NaN, a fraction, out of range — leaves loop_end 0, and the node fails activation at the next update; D = 0
            // is a valid delay, so the marker is D + 1
            const bool ok = d >= 0.0f && d <= (float)DCOMP_MAX && d == floorf(d);
            s.loop_start = ok ? (uint64_t)d : 0;
            s.loop_end = ok ? (uint64_t)d + 1 : 0;
            break;
        }
        case K_CROSSFADE: {  // params: position (0..1, default 0: all A), law (0 linear, 1 equal power; default 1)
            const float pos = p(0, 0.0f), law = p(1, (float)XF_LAW_EQUAL_POWER);
            // anything else — NaN, out of range, another law — leaves loop_end 0, and the node fails activation at the next update
            const bool ok = pos >= 0.0f && pos <= 1.0f && (law == (float)XF_LAW_LINEAR || law == (float)XF_LAW_EQUAL_POWER);
            s.p0 = s.p1 = ok ? pos : 0.0f;  // at rest at `position`: dur (full_range) 0, t0 (loop_start) 0, node time (playhead) 0
            s.playing = ok ? (int)law : XF_LAW_EQUAL_POWER;
            s.has_loop = XF_SHAPE_LINEAR;
            s.loop_end = ok ? 1 : 0;
            break;
        }
        default:
            break;
    }
    return s;
}

}  // namespace fwgpu
