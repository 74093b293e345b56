// fwgpu_types.h — POD structs shared by the host planner and the HIP kernels (HBM-resident layout).
#pragma once
#include <math.h>
#include <stdint.h>

namespace fwgpu {

enum : int {
    K_DUMMY = 0, K_BEEP = 1, K_VOLUME = 2, K_SUM = 3, K_SAMPLER = 4, K_HARD_CLIP = 5,
    K_MONO_TO_STEREO = 6, K_STEREO_TO_MONO = 7, K_PAN = 8, K_WIDTH = 9, K_BIQUAD = 10, K_DELAY = 11,
    K_FIR = 12, K_RESAMPLER = 13, K_SPATIAL = 14,
    K_HOST = 15,  // a node the library does not implement: the caller's own AudioNodeProcessor::process, run on the host
    K_METER = 16,  // SPEC level meter: per block and input channel peak, sum of squares and overs; audio passes through
    K_LIMITER = 17,  // SPEC look-ahead limiter: linked channels, sliding minimum + 64-term moving average, 63 frames of latency
    K_DUCKER = 18,  // SPEC sidechain ducker: n main + k key inputs, n outputs; window counts of the key's gate bits, no latency
    K_DELAY_COMP = 19,  // SPEC latency compensation: n -> n, a pure delay of a whole number of frames, a copy with no arithmetic
    K_CROSSFADE = 20,  // SPEC crossfader: 2n -> n, two buses blended along an automated curve of the node's frame count; k_level<0> renders it
    K_LAST = K_CROSSFADE,  // the last node kind that k_level renders and a message may reach (the kinds behind it bring a kernel of their own)
    K_COMPRESSOR = 21,  // SPEC bus compressor: n -> n, self-keyed, linked channels; a table curve and window sums of the gain target, no latency
    K_KIND_MAX = K_COMPRESSOR,  // the last node kind fwgpu_add_node accepts
};
#if defined(__HIPCC__)
#define FW_TYPES_HD __host__ __device__
#else
#define FW_TYPES_HD  // (the test harnesses compile the host translation units with plain g++)
#endif
#define FW_TYPES_HD_INLINE FW_TYPES_HD inline __attribute__((always_inline))
// Raw bits in a field of another type — how integers travel in NodeState's float slots and in a message's doubles (the Cmd makers
// and readers below).  A pair of floats in a double: `lo` in bits 0..31, `hi` in bits 32..63.
FW_TYPES_HD constexpr uint32_t fw_bits_of(float f) { return __builtin_bit_cast(uint32_t, f); }
FW_TYPES_HD constexpr float fw_float_of(uint32_t u) { return __builtin_bit_cast(float, u); }
FW_TYPES_HD constexpr uint64_t fw_bits_of64(double d) { return __builtin_bit_cast(uint64_t, d); }
FW_TYPES_HD constexpr double fw_double_of(uint64_t u) { return __builtin_bit_cast(double, u); }
FW_TYPES_HD constexpr double fw_double_of2(float lo, float hi) { return fw_double_of((uint64_t)fw_bits_of(lo) | ((uint64_t)fw_bits_of(hi) << 32)); }
FW_TYPES_HD constexpr float fw_lo_float_of(double d) { return fw_float_of((uint32_t)fw_bits_of64(d)); }
FW_TYPES_HD constexpr float fw_hi_float_of(double d) { return fw_float_of((uint32_t)(fw_bits_of64(d) >> 32)); }
// Which kernel runs a kind.  The node kernel k_level exists in three instantiations, by register appetite: one kernel for every kind
// needed 248 VGPRs (2 waves per SIMD — nothing to hide HBM latency behind, 0.9 TB/s on a level of volume nodes).  Set 0: the streaming
// kinds (volume, pan, sum, hard clip, mono<->stereo, width: 127 VGPRs), set 1: serial recurrences / filter banks / libm (beep, biquad,
// delay, resampler, spatialiser: 147), set 2: the sampler (every sample format, wraps, tails, ramps).  Sets 4 and above are no
// instantiation of k_level: a kernel of its own, launched next to them (k_limiter, k_ducker, k_delay_comp, k_compressor).
FW_TYPES_HD inline int kind_set(int kind) {
    if (kind == K_SAMPLER) return 2;
    if (kind == K_LIMITER) return 4;
    if (kind == K_DUCKER) return 5;
    if (kind == K_DELAY_COMP) return 6;
    if (kind == K_COMPRESSOR) return 7;
    return (kind == K_BEEP || kind == K_BIQUAD || kind == K_DELAY || kind == K_RESAMPLER || kind == K_SPATIAL) ? 1 : 0;
}
FW_TYPES_HD inline bool kind_has_own_kernel(int kind) { return kind_set(kind) >= 4; }
// a level's launch bits (launch_level's `kinds`): bit s = the level holds a kind of set s, plus LB_WALKERS for a biquad / delay (in a
// batch, the ones that are bus effects go to the walkers' kernel k_bus_iir)
enum : int { LB_SET0 = 1, LB_SET1 = 2, LB_SET2 = 4, LB_WALKERS = 8, LB_LIMITER = 16, LB_DUCKER = 32, LB_DELAY_COMP = 64, LB_COMPRESSOR = 128 };
FW_TYPES_HD inline int kind_launch_bits(int kind) { return (1 << kind_set(kind)) | ((kind == K_BIQUAD || kind == K_DELAY) ? LB_WALKERS : 0); }
static_assert(LB_LIMITER == 1 << 4 && LB_DUCKER == 1 << 5 && LB_DELAY_COMP == 1 << 6 && LB_COMPRESSOR == 1 << 7, "a launch bit is 1 << kind_set");
// K_CROSSFADE: n output channels (bus A on inputs 0..n-1, bus B on n..2n-1), the longest segment in frames (2^24: k and dur convert to
// f32 exactly), the bisection steps of the Bezier solver, and the two laws / shapes
#define XF_CH_MAX 8
#define XF_FRAMES_MAX 16777216u
#define XF_ITERS 24
#define XF_LAW_LINEAR 0
#define XF_LAW_EQUAL_POWER 1
#define XF_SHAPE_LINEAR 0
#define XF_SHAPE_BEZIER 1
// K_DELAY_COMP: the delay D is a whole number of frames in 0..DCOMP_MAX.  The node's ext slice keeps the last D input frames per channel
// and, behind them, one counter per channel (the silence rule's loud_c) in a 32-bit slot each.
#define DCOMP_MAX 8192u
#define DCOMP_CH_MAX 8
#define DCOMP_DEFAULT 63u
// K_DUCKER: the caps of attack, release and hold (frames).  The gate's history is W = max(A, R) + H bits, at most DUCK_WIN_MAX +
// DUCK_HOLD_MAX = 65 536 bits = 8 KiB, and a wave stages it in LDS in front of the DUCK_RUN_MAX frames (1 KiB of bits) it renders:
// the caps are sized so that the staged bit window stays around 10 KB of LDS (k_ducker.hip.h DuckLds).
#define DUCK_WIN_MAX 32768u
#define DUCK_HOLD_MAX 32768u
#define DUCK_RUN_MAX 8192
#define DUCK_CH_MAX 8
#define DUCK_THRESHOLD_DEFAULT 0.05f
#define DUCK_DEPTH_DEFAULT 0.25f
#define DUCK_ATTACK_DEFAULT 480u
#define DUCK_RELEASE_DEFAULT 12000u
#define DUCK_HOLD_DEFAULT 4800u
// K_COMPRESSOR: the caps of attack / release and of hold (frames) and of the channel count.  The node's ext slice holds the gain table
// G[0..COMP_TAB_N) (16 knots per octave over 20 octaves above T0, and the knot that ends them) padded to COMP_TAB_PAD floats and, behind
// it, the last W = max(A, R) + H values of 65535 - q as 16-bit words, oldest first, two to a 32-bit slot.  A workgroup stages W + run
// of them in LDS: COMP_RUN_MAX is sized so that two workgroups share a CU's 160 KiB (k_compressor.hip.h CompLds).
#define COMP_WIN_MAX 32768u
#define COMP_HOLD_MAX 2048u
#define COMP_RUN_MAX 4096
#define COMP_CH_MAX 8
#define COMP_TAB_N 321
#define COMP_TAB_PAD 328
#define COMP_OCTAVES 20
#define COMP_THRESHOLD_DEFAULT 0.25f
#define COMP_RATIO_DEFAULT 4.0f
#define COMP_KNEE_DEFAULT 6.0f
#define COMP_ATTACK_DEFAULT 240u
#define COMP_RELEASE_DEFAULT 12000u
#define COMP_HOLD_DEFAULT 0u
#define COMP_MAKEUP_DEFAULT 1.0f
// K_LIMITER: LIM_LOOK terms in the moving average (one per lane of a wave; 1/64 is an exact scale), latency LIM_LOOK - 1 frames.  The
// node's ext slice keeps the last H + LIM_HIST_PAD input frames per channel (H = hold_frames); a block reads back H + 2 * (LIM_LOOK - 1).
#define LIM_LOOK 64
#define LIM_HOLD_DEFAULT 128u
#define LIM_HOLD_MAX 1920u
#define LIM_HIST_PAD 128u
#define LIM_CH_MAX 8
// K_METER: one record per (block, input channel) — include/fwgpu.h fwgpu_meter_reading, written as ONE 16-byte store.  The node's
// ext slice is a ring of R x n_in of them (R = NodeState::loop_end); block g of the ctx's block count sits in slot g % R.
struct MeterRec {
    float peak, sum_squares;
    uint32_t over, frames;
};
static_assert(sizeof(MeterRec) == 16, "MeterRec layout");
#define METER_RING_DEFAULT 1024u
#define METER_RING_MAX 65536u
// K_METER, spectrum meter (SPEC): a meter created with two or more parameters also records, per (block, input channel),
// the band powers of a Hann-windowed radix-2 FFT over the channel's last N frames.  N is a power of two in SPEC_FFT_MIN..SPEC_FFT_MAX,
// `bands` 0 (every bin, DC included: N/2 + 1 values per record) or 1..N/2 (log-spaced bands over bins 1..N/2), at most SPEC_CH_MAX
// channels, and the spectrum ring holds at most SPEC_RING_FLOATS_MAX floats (the largest plain meter ring).
#define SPEC_FFT_MIN 256u
#define SPEC_FFT_MAX 4096u
#define SPEC_CH_MAX 8
#define SPEC_BANDS_DEFAULT 32u
#define SPEC_RING_FLOATS_MAX 16777216u
#define RS_PHASES 32  // SPEC resampler: polyphase windowed-sinc table [RS_PHASES][RS_TAPS], 32.32 fixed-point position
#define RS_TAPS 16
// realtime edge, resident kernel (k_rt_persist): the mailbox in pinned, device-mapped host memory
struct RtMailbox {
    unsigned long long doorbell;  // host -> device: the sequence number to render next, or that number | RT_QUIT_BIT
    unsigned long long hold;      // host (CONTROL side) -> device: > 0 while a control call is about to free device memory or wait for the
                                  // device (hipFree synchronises with every stream — a kernel that never ends would hold it forever):
                                  // the kernel ends as if its watchdog had fired, and the audio side launches no new one (RtHold)
    unsigned long long pad0[6];
    unsigned long long alive;     // device -> host: 1 while the kernel takes doorbells, 0 once it has decided to end
    unsigned long long pad1[7];
};
#define RT_QUIT_BIT (1ull << 63)
#define RT_PREFETCH_BIT (1ull << 62)  // device-internal (`go` word): "no doorbell for 10 us: fetch the next block's sources now"
#define LEAF_WPB_MAX 4  // k_leaf.hip.h: at most this many 256-frame pieces (waves) per block
#define SP_HIST 64    // SPEC spatialiser: mono history frames (>= the largest per-ear delay + 1)

enum : int { FMT_I_I16 = 0, FMT_I_U16 = 1, FMT_I_F32 = 2, FMT_P_I16 = 3, FMT_P_U16 = 4, FMT_P_F32 = 5 };

// core/param/smoother.rs:72-88 without the output Vec: whenever status != Active the reference's buffer
// is constant == input (every path that leaves Active fills it), so only the scalars are state.
enum : int { SM_INACTIVE = 0, SM_ACTIVE = 1, SM_DEACTIVATING = 2 };
struct Smoother {
    int status;
    float input;
    float last;  // last_output
    float a, b, eps;
};

// One state record per node (audio half of every node kind; 128 B, indexed by node slot).
struct NodeState {
    float p0, p1;  // the reference's atomics: VOLUME/SAMPLER raw_gain; PAN gl,gr targets; HARD_CLIP threshold
    Smoother s0, s1;
    // nodes/sampler.rs:280-292
    int playing;
    int has_loop;
    int full_range;
    int sample;  // sample-table index, -1 = None
    uint64_t playhead;
    uint64_t loop_start, loop_end;
    // nodes/beep_test.rs:64-69
    float phasor, phasor_inc, gain;
    int enabled;
    uint32_t sample_rate;
    // SPEC nodes with per-channel state: offset/length (floats) of this node's slice of the ext pool
    //   BIQUAD: ext = [b0 b1 b2 a1 a2][x1 x2 y1 y2] x channels      DELAY: ext = ring[channels][D]
    //   BIQUAD also keeps its coefficient sweep (CMD_BQ_SWEEP) in the two smoothers, which it has no other use for:
    //        s0.status = N (0: at rest, the coefficients are the ext head's), s1.status = k, s0 / s1 .input .last .a .b .eps = A / T
    //        (bq_sweep_* below the struct); behind the channels' state the ext slice holds BQ_SNAP_LEN more floats, the sweep as
    //        it stood at the START of the chain plan's current call (k_voice_control writes it, k_chain's sweep instantiation reads it)
    //   DELAY also uses p0 = feedback, p1 = mix, gain = dry (1-mix), playhead = ring position, loop_end = D
    //   FIR: ext = mirrored history ring[channels][2R]; playhead = ring position, loop_end = R, loop_start = T,
    //        sample = impulse-response sample id (a morph-capable node: of slot A at activation; enabled = 1 and the fields listed
    //        at fir_morph_* below hold its segment, node time and block records)
    //   SAMPLER also keeps its gain envelope (CMD_SMP_FADE) in fields it has no other use for: phasor = E0, gain = E1,
    //        enabled = N in bits 0..24 and `then` (SMP_FADE_*) in bits 28..29, s1.status = k (frames of the fade rendered, k < N).
    //        At rest: enabled == 0 and s1.status == 0, the value is E1 = gain.  make_state leaves a new sampler at rest at 1.0f; no
    //        message but CMD_SMP_FADE reaches these fields (a sampler's only parameter is p0); a node's state keeps its slot over
    //        a plan install (only the steady cache is carried, and a voice in a fade has none), and k_lazy_flush moves the playhead alone — a voice in a fade leaves no lazy record.  The arithmetic is
    //        smp_env_* below the struct
    //   SAMPLER on a stream (CMD_SMP_STREAM) also keeps W, C, E, U and its flags as raw bits in ext_off / ext_len, s1.input /
    //        s1.last, s1.a / s1.b, aux and phasor_inc (a sampler has no ext slice and no second smoother), with has_loop = 1 and
    //        loop = [0, R): smp_stream_* below the struct.  A sampler that holds no stream has phasor_inc == 0 (make_state)
    //   RESAMPLER: sample = source, playhead = 32.32 source position, loop_start = 32.32 step, has_loop, playing; a ratio glide
    //        (CMD_RS_GLIDE): full_range = left (frames of the glide still to render, 0: none), loop_end = target (the
    //        step behind the glide), enabled / ext_off = the low / high 32 bits of inc, the signed step change per frame (a
    //        resampler has no ext slice: ext_len stays 0).  make_state leaves all four 0; the arithmetic is rs_glide_* below the struct
    //   SPATIAL: p0/p1 = ear gain targets (s0/s1 smooth them), playing = left-ear delay, has_loop = right-ear delay
    //        (frames), ext = the last SP_HIST mono samples; a move (CMD_SP_MOVE) in fields it has no other use for:
    //        full_range = N (0: at rest), enabled = k (frames of the move rendered, k < N), phasor / phasor_inc = G0l / G0r, playhead /
    //        loop_start = Dl / Dr (the 32.32 per-ear delays at the NEXT block's first frame), loop_end = inc_l, sample | gain bits << 32
    //        = inc_r (signed, as two's-complement bits).  In a move p0 / p1 and both smoothers rest at the target gains and playing /
    //        has_loop hold the target delays: the move's end only clears N and k.  make_state leaves N = k = 0 (the device copy of
    //        phasor / phasor_inc / gain then holds the constructor's x / y / z, which no kernel reads; the host keeps its own in
    //        HostNode::init); a node's state keeps its slot over a plan install.  The arithmetic is sp_move_* below the struct
    //   VOLUME, PAN: a gain ride (CMD_GAIN_RIDE) in fields neither kind has another use for, ONE layout for both:
    //        full_range = N (0: at rest), enabled = k (frames of the ride rendered, k < N), phasor / phasor_inc = G0_0 / G0_1 (a volume:
    //        G0_1 = 0), has_loop = shape (XF_SHAPE_*), playhead = x1 bits | y1 bits << 32, loop_start = x2 bits | y2 bits << 32.  In a
    //        ride p0 / p1 and both smoothers rest at the targets G1_0 / G1_1 (a volume's p1 and s1 stay at 0, as make_state leaves
    //        them): the ride's end only clears these seven fields, back to make_state's zeros.  No other message reaches them; a
    //        node's state keeps its slot over a plan install.  The arithmetic is gain_ride_* below the struct
    //   METER: ext = ring[R][n_in] of MeterRec (4 floats each), loop_end = R (0: the creation parameter was refused); a spectrum meter
    //        also has loop_start = N, full_range = bands, playing = B and a longer slice: spec_state_ok / spec_ext_len below the struct
    //   LIMITER, DUCKER, DELAY_COMP, COMPRESSOR: loop_end = 0 marks a creation parameter that was refused; the valid states and the
    //        slice lengths are lim_/duck_/dcomp_/comp_state_ok and _ext_len below the struct
    //   LIMITER: p0 = ceiling C, loop_start = hold_frames H, loop_end = HK; ext = hist[n_in][HK]: the last HK input frames per channel,
    //        oldest first
    //   DUCKER: p0 = threshold T, p1 = depth D, playhead = A, loop_start = R, full_range = H, loop_end = W; ext = the last W gate bits
    //        on[], oldest first, bit i in bit i % 32 of word i / 32 (the float slots hold 32-bit words), the bits from W on zero
    //   COMPRESSOR: p0 = T0 (where the knee begins), p1 = makeup M, playhead = A, loop_start = R, full_range = H, loop_end = W; phasor_inc,
    //        gain, phasor = the creation parameters threshold, ratio, knee_db (the host builds the table from them at activation; no
    //        kernel reads them); ext = G[COMP_TAB_PAD], then the last W values of 65535 - q as 16-bit words, oldest first, value i in
    //        bits 16 * (i % 2) of slot COMP_TAB_PAD + i / 2 — zeros, as every slice starts, are the SPEC's unity history
    //   DELAY_COMP: loop_start = D, loop_end = D + 1; ext = hist[n_in][D]: the last D input frames per channel, oldest first (a block
    //        flagged silent enters as zeros), then loud[n_in]: 32-bit counters in the float slots — how many of the frames in front of
    //        the next block may still be heard
    //   CROSSFADE: no ext slice.  playhead = node time T (frames rendered since activation), p0 = P0, p1 = P1, loop_start = t0,
    //        full_range = dur (0: at rest at P1), has_loop = shape (XF_SHAPE_*), phasor, phasor_inc, gain, aux = x1, y1, x2, y2,
    //        playing = law (XF_LAW_*), loop_end = 1 (0: a creation parameter was refused); the valid states are xf_state_ok
    uint32_t ext_off;
    uint32_t ext_len;
    float aux;  // CROSSFADE: y2; every other kind: 0
};
static_assert(sizeof(NodeState) == 128, "NodeState layout");
// The bus nodes with a kernel of their own: the states their kernels render (anything else would index the ext slice out of bounds)
// and the length of that slice, in floats.  ONE statement for the plan build (activate_nodes refuses what fails), the device guards and
// the host harness (tests/host_harness/launch_stubs.cpp); make_state is what fills the fields.
FW_TYPES_HD inline bool lim_state_ok(const NodeState& s, int n_in, int n_out) {
    const uint64_t H = s.loop_start;
    return H <= LIM_HOLD_MAX && s.loop_end == H + LIM_HIST_PAD && n_in == n_out && n_in >= 1 && n_in <= LIM_CH_MAX;
}
FW_TYPES_HD inline uint32_t lim_ext_len(const NodeState& s, int n_in) { return (uint32_t)n_in * (uint32_t)s.loop_end; }
// (n_out main channels, n_in - n_out key channels; W = max(A, R) + H gate bits in 64-bit groups)
FW_TYPES_HD inline bool duck_state_ok(const NodeState& s, int n_in, int n_out) {
    const uint64_t A = s.playhead, R = s.loop_start, W = s.loop_end;
    const int H = s.full_range;
    return A >= 1 && A <= DUCK_WIN_MAX && R >= 1 && R <= DUCK_WIN_MAX && H >= 0 && H <= (int)DUCK_HOLD_MAX &&
           W == (A > R ? A : R) + (uint64_t)H && n_out >= 1 && n_out <= DUCK_CH_MAX && n_in - n_out >= 1 && n_in - n_out <= DUCK_CH_MAX;
}
FW_TYPES_HD inline uint32_t duck_ext_len(const NodeState& s) { return 2u * (uint32_t)((s.loop_end + 63) / 64); }
FW_TYPES_HD inline bool dcomp_state_ok(const NodeState& s, int n_in, int n_out) {
    const uint64_t D = s.loop_start;
    return D <= DCOMP_MAX && s.loop_end == D + 1 && n_in == n_out && n_in >= 1 && n_in <= DCOMP_CH_MAX;
}
FW_TYPES_HD inline uint32_t dcomp_ext_len(const NodeState& s, int n_in) { return (uint32_t)n_in * (uint32_t)s.loop_start + (uint32_t)n_in; }
// (n -> n; the table, then W = max(A, R) + H 16-bit words in 32-bit slots)
FW_TYPES_HD inline bool comp_state_ok(const NodeState& s, int n_in, int n_out) {
    const uint64_t A = s.playhead, R = s.loop_start, W = s.loop_end;
    const int H = s.full_range;
    return A >= 1 && A <= COMP_WIN_MAX && R >= 1 && R <= COMP_WIN_MAX && H >= 0 && H <= (int)COMP_HOLD_MAX &&
           W == (A > R ? A : R) + (uint64_t)H && n_in == n_out && n_in >= 1 && n_in <= COMP_CH_MAX && s.p0 > 0.0f && s.p1 > 0.0f;
}
FW_TYPES_HD inline uint32_t comp_ext_len(const NodeState& s) { return (uint32_t)COMP_TAB_PAD + (uint32_t)((s.loop_end + 1) / 2); }
// K_METER, spectrum meter: loop_end = R as for every meter, loop_start = N (0: a plain meter, whose state and slice are what they
// were), full_range = the `bands` parameter, playing = B, the floats of one record (bands, or N/2 + 1 when bands == 0).  The slice, every
// part at a multiple of 64 floats: the level ring a plain meter has (k_level and fwgpu_meter_read find it at ext_off, as ever), the window
// w[N], the twiddles wr[N/2] wi[N/2], the edges e[B + 1] as 32-bit words, hist[n_in][N]: the last N input frames per channel, oldest
// first (zeros at activation: the SPEC's x[n < 0]), and the spectrum ring [R][n_in][B].  The host uploads window, twiddles and edges
// (fwgpu_control_math.cpp spectrum_tables) as the slice's `head`, spec_head_len floats from spec_win_rel on.
FW_TYPES_HD inline bool spec_on(const NodeState& s) { return s.loop_start != 0; }
FW_TYPES_HD inline bool spec_state_ok(const NodeState& s, int n_in, int n_out) {
    const uint64_t R = s.loop_end, N = s.loop_start;
    const uint32_t bands = (uint32_t)s.full_range, B = (uint32_t)s.playing;
    return R >= 1 && R <= METER_RING_MAX && N >= SPEC_FFT_MIN && N <= SPEC_FFT_MAX && (N & (N - 1)) == 0 && s.full_range >= 0 && bands <= N / 2 &&
           B == (bands ? bands : (uint32_t)N / 2 + 1) && n_in >= 1 && n_in <= SPEC_CH_MAX && (n_out == n_in || n_out == 0) &&
           R * (uint64_t)n_in * B <= SPEC_RING_FLOATS_MAX;
}
FW_TYPES_HD inline uint32_t spec_win_rel(const NodeState& s, int n_in) { return ((uint32_t)s.loop_end * (uint32_t)n_in * 4u + 63u) / 64u * 64u; }
FW_TYPES_HD inline uint32_t spec_tw_rel(const NodeState& s, int n_in) { return spec_win_rel(s, n_in) + (uint32_t)s.loop_start; }
FW_TYPES_HD inline uint32_t spec_edges_rel(const NodeState& s, int n_in) { return spec_win_rel(s, n_in) + 2u * (uint32_t)s.loop_start; }
FW_TYPES_HD inline uint32_t spec_head_len(const NodeState& s) { return 2u * (uint32_t)s.loop_start + ((uint32_t)s.playing + 1u + 63u) / 64u * 64u; }
FW_TYPES_HD inline uint32_t spec_hist_rel(const NodeState& s, int n_in) { return spec_win_rel(s, n_in) + spec_head_len(s); }
FW_TYPES_HD inline uint32_t spec_ring_rel(const NodeState& s, int n_in) { return spec_hist_rel(s, n_in) + (uint32_t)n_in * (uint32_t)s.loop_start; }
FW_TYPES_HD inline uint32_t spec_ext_len(const NodeState& s, int n_in) {
    return spec_ring_rel(s, n_in) + (uint32_t)s.loop_end * (uint32_t)n_in * (uint32_t)s.playing;
}

// A ramp: a value moved from a to b over N frames by one message.  The frame at position u in [0, 1) is a + (d * u),
// d = b - a (callers hoist it), each a separately rounded f32 operation (-ffp-contract=off).  The clamp: a + d can round one ulp past
// b, and a curve that overshoots may put u outside [0, 1] — the value stays inside [min(a, b), max(a, b)].  Where u comes from is
// each feature's own: (k + j) / N for a fade, a sweep (one division for its five coefficients) and a move, the curve's y for a ride.
FW_TYPES_HD_INLINE float fw_ramp_mix(float a, float b, float d, float u) {
    const float v = a + (d * u);
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    return v < lo ? lo : (v > hi ? hi : v);
}
// A 32.32 number moved from `from` to `to` over N frames: the signed increment per frame, truncated toward zero — N steps of it stay
// between the two ends, and the ramp's last frame is followed by exactly `to`.  Wrapping u64 arithmetic; the signed inc travels as
// its two's-complement bits.  N != 0
FW_TYPES_HD_INLINE uint64_t fw_glide_inc(uint64_t from, uint64_t to, uint32_t N) { return (uint64_t)((int64_t)(to - from) / (int64_t)N); }

// K_RESAMPLER ratio glide (SPEC): ONE statement for the node kernels, the control kernel and the leaf kernel.  All in
// wrapping u64 arithmetic; a signed inc travels as its two's-complement bits.
#define RS_GLIDE_FRAMES_MAX 16777216u
FW_TYPES_HD inline uint64_t rs_glide_inc(const NodeState& s) { return ((uint64_t)s.ext_off << 32) | (uint64_t)(uint32_t)s.enabled; }
// the message, applied at a block's first frame: N frames from the step the node has reached to S1 (N == 0: a step)
FW_TYPES_HD inline void rs_glide_start(NodeState& s, uint64_t S1, uint32_t N) {
    // (N == 0 is the SPEC's step.  N > RS_GLIDE_FRAMES_MAX is NOT SPEC behaviour: fwgpu_resampler_glide refuses such a call, so only a
    //  corrupted message gets here — a defensive branch that keeps `left` inside its 2^24 and the division's operands in range)
    if (N == 0u || N > RS_GLIDE_FRAMES_MAX) {
        s.loop_start = S1;
        s.full_range = 0;
        return;
    }
    const uint64_t inc = fw_glide_inc(s.loop_start, S1, N);
    s.enabled = (int)(uint32_t)inc;
    s.ext_off = (uint32_t)(inc >> 32);
    s.full_range = (int)N;
    s.loop_end = S1;
}
// 32.32 position of frame i of a run that starts at (pos0, step0) with `left` frames of the glide to go (left == 0: no glide, the
// step is step0 throughout); frames behind the glide's end move by `target`
FW_TYPES_HD inline uint64_t rs_glide_pos(uint64_t pos0, uint64_t step0, uint64_t inc, uint64_t left, uint64_t target, uint64_t i) {
    const uint64_t m = i < left ? i : left;
    const uint64_t tri = (m * (m - 1ull)) >> 1;  // m (m - 1) / 2 < 2^47 (m == 0: 0 x anything)
    return pos0 + m * step0 + inc * tri + (i - m) * (left ? target : step0);
}
// the state behind a rendered block of `frames` frames (the position is rs_glide_pos(..., frames), taken BEFORE this)
FW_TYPES_HD inline void rs_glide_advance(NodeState& s, uint32_t frames) {
    const uint32_t left = (uint32_t)s.full_range;
    if (left == 0u) return;
    if (frames >= left) {
        s.loop_start = s.loop_end;  // exactly the target
        s.full_range = 0;
    } else {
        s.loop_start += (uint64_t)frames * rs_glide_inc(s);
        s.full_range = (int)(left - frames);
    }
}
// A VB_RS_GLIDE block's record (VoiceBlk): off0 / off1 = position / step of frame 0; src_r bits = inc in the low 41 bits (|inc| <
// 2^40) and min(left, RS_GLIDE_LEFT_CAP) above them; n1 = the loop flag in bit 0 and, above it, target - (off1 + left x inc) + 2^24
// — the remainder of the truncated division, below 2^24 in magnitude — from which a block the glide ends in rebuilds the target.
// A block has fewer than RS_GLIDE_LEFT_CAP frames, so a capped `left` never ends inside one.
#define RS_GLIDE_LEFT_CAP 0x7fffffu
FW_TYPES_HD inline uint64_t rs_glide_pack(const NodeState& s) {
    const uint32_t left = (uint32_t)s.full_range;
    return (rs_glide_inc(s) & ((1ull << 41) - 1)) | ((uint64_t)(left < RS_GLIDE_LEFT_CAP ? left : RS_GLIDE_LEFT_CAP) << 41);
}
FW_TYPES_HD inline uint32_t rs_glide_rem(const NodeState& s) {
    return (uint32_t)(s.loop_end - (s.loop_start + (uint64_t)(uint32_t)s.full_range * rs_glide_inc(s)) + (1ull << 24));
}
FW_TYPES_HD inline void rs_glide_unpack(uint64_t bits, uint32_t n1, uint64_t step0, uint64_t& inc, uint64_t& left, uint64_t& target) {
    inc = (uint64_t)((int64_t)(bits << 23) >> 23);
    left = bits >> 41;
    target = step0 + left * inc + (uint64_t)(n1 >> 1) - (1ull << 24);
}

// K_SAMPLER gain envelope (SPEC): ONE statement for the message (apply_cmds_from), the node kernels and the control
// kernel.  E0 -> E1 over N frames, k of them rendered; at rest (N == 0) the value is E1.  Every operation below is a separately rounded
// f32 operation (-ffp-contract=off), the division is IEEE, and (float)(k + j), (float)N are exact (both <= 2^24).
#define SMP_FADE_FRAMES_MAX 16777216u
#define SMP_FADE_NONE 0
#define SMP_FADE_PAUSE 1
#define SMP_FADE_STOP 2
FW_TYPES_HD inline uint32_t smp_env_N(const NodeState& s) { return (uint32_t)s.enabled & 0x1ffffffu; }
FW_TYPES_HD inline int smp_env_then(const NodeState& s) { return (s.enabled >> 28) & 3; }
FW_TYPES_HD inline bool smp_env_at_rest(const NodeState& s) { return smp_env_N(s) == 0u; }
// the envelope as a block's render loop reads it: a snapshot taken BEFORE the block's advance, d = E1 - E0 computed once
struct SmpEnv {
    float E0, E1, d;
    uint32_t N, k;
};
FW_TYPES_HD inline SmpEnv smp_env_of(const NodeState& s) {
    SmpEnv e;
    e.E0 = s.phasor;
    e.E1 = s.gain;
    e.d = e.E1 - e.E0;
    e.N = smp_env_N(s);
    e.k = (uint32_t)s.s1.status;
    return e;
}
// env(j): the value of the frame j frames ahead of the snapshot's position
FW_TYPES_HD inline float smp_env_value(const SmpEnv& e, uint32_t j) {
    const uint32_t t = e.k + j;
    if (e.N == 0u || t >= e.N) return e.E1;
    return fw_ramp_mix(e.E0, e.E1, e.d, (float)t / (float)e.N);
}
FW_TYPES_HD inline void smp_env_reset(NodeState& s) {  // the envelope is a transient: at rest at 1.0f, then = NONE
    s.gain = 1.0f;
    s.enabled = 0;
    s.s1.status = 0;
}
// the message, applied at a block's first frame: `frames` frames from where the envelope stands to `target` (frames == 0: a step)
FW_TYPES_HD inline void smp_env_start(NodeState& s, float target, uint32_t frames, int then) {
    // (frames > SMP_FADE_FRAMES_MAX or a `then` outside 0..2 is NOT SPEC behaviour: fwgpu_sampler_fade refuses such a call, so only a
    //  corrupted message gets here — a defensive branch that keeps k and N inside their 2^24)
    if (frames == 0u || frames > SMP_FADE_FRAMES_MAX || then < SMP_FADE_NONE || then > SMP_FADE_STOP) {
        s.gain = target;
        s.enabled = 0;
        s.s1.status = 0;
        return;
    }
    s.phasor = smp_env_value(smp_env_of(s), 0u);  // a retarget in mid-fade continues from where the fade stands
    s.gain = target;
    s.enabled = (int)(frames | ((uint32_t)then << 28));
    s.s1.status = 0;
}
// K_SAMPLER on a stream (SPEC streaming source): ONE statement for the messages (apply_cmds_from), the node kernels and
// the control kernel.  The sample is a ring of R frames the control side appends to; the sampler is a looping sampler over the whole
// ring (has_loop = 1, loop = [0, R): smp_stream_bind sets the fields, no loop or seek message moves them while the stream is on) and
// keeps four integers in fields a sampler has no other use for, as raw bits: W (frames written that it has been told of) in
// ext_off | ext_len << 32, C (frames consumed) in s1.input | s1.last << 32, E (the end; valid with SMP_STREAM_HAS_END) in
// s1.a | s1.b << 32, U (starved blocks) in aux, the flags in phasor_inc.  A sampler that holds no stream has flags == 0.
#define SMP_STREAM_ON 1u
#define SMP_STREAM_HAS_END 2u
#define SMP_STREAM_FINISHED 4u
#define SMP_STREAM_RING_MAX (1ull << 30)
#define SMP_STREAM_RING_MIN_BLOCKS 4u
struct SmpStream {
    uint64_t W, C, E;
    uint32_t U, flags;
};
FW_TYPES_HD inline uint32_t smp_stream_flags(const NodeState& s) { return fw_bits_of(s.phasor_inc); }
FW_TYPES_HD inline bool smp_stream_on(const NodeState& s) { return (smp_stream_flags(s) & SMP_STREAM_ON) != 0u; }
FW_TYPES_HD inline bool smp_stream_finished(const NodeState& s) { return (smp_stream_flags(s) & SMP_STREAM_FINISHED) != 0u; }
// the voice reads a ring that may be written under it: never steady, never frozen, no lazy record — until the stream is finished
FW_TYPES_HD inline bool smp_stream_live(const NodeState& s) { return (smp_stream_flags(s) & (SMP_STREAM_ON | SMP_STREAM_FINISHED)) == SMP_STREAM_ON; }
FW_TYPES_HD inline SmpStream smp_stream_of(const NodeState& s) {
    SmpStream t;
    t.W = (uint64_t)s.ext_off | ((uint64_t)s.ext_len << 32);
    t.C = (uint64_t)fw_bits_of(s.s1.input) | ((uint64_t)fw_bits_of(s.s1.last) << 32);
    t.E = (uint64_t)fw_bits_of(s.s1.a) | ((uint64_t)fw_bits_of(s.s1.b) << 32);
    t.U = fw_bits_of(s.aux);
    t.flags = smp_stream_flags(s);
    return t;
}
FW_TYPES_HD inline void smp_stream_put(NodeState& s, const SmpStream& t) {
    s.ext_off = (uint32_t)t.W;
    s.ext_len = (uint32_t)(t.W >> 32);
    s.s1.input = fw_float_of((uint32_t)t.C);
    s.s1.last = fw_float_of((uint32_t)(t.C >> 32));
    s.s1.a = fw_float_of((uint32_t)t.E);
    s.s1.b = fw_float_of((uint32_t)(t.E >> 32));
    s.aux = fw_float_of(t.U);
    s.phasor_inc = fw_float_of(t.flags);
}
// CMD_SMP_SET_SAMPLE with a stream (R = the ring's frames, W = the frames written so far): the sampler starts at the ring's frame 0
FW_TYPES_HD inline void smp_stream_bind(NodeState& s, uint64_t R, uint64_t W) {
    SmpStream t;
    t.W = W;
    t.C = t.E = 0;
    t.U = 0;
    t.flags = SMP_STREAM_ON;
    smp_stream_put(s, t);
    s.has_loop = 1;
    s.full_range = 0;
    s.loop_start = 0;
    s.loop_end = R;
    s.playhead = 0;
}
// CMD_SMP_SET_SAMPLE with anything else on a sampler that holds a stream: a one-shot at frame 0 again
FW_TYPES_HD inline void smp_stream_unbind(NodeState& s) {
    SmpStream t;
    t.W = t.C = t.E = 0;
    t.U = 0;
    t.flags = 0;
    smp_stream_put(s, t);
    s.has_loop = 0;
    s.full_range = 0;
    s.loop_start = s.loop_end = 0;
    s.playhead = 0;
}
// CMD_SMP_STREAM: W (never backwards), and with `has_end` the end E; ignored by a sampler that holds no stream.  An end that arrives
// when every frame has been played already (E <= C: the writer called `end` late) finishes the sampler here, as the block that reached E
// would have (smp_pause): no block of padding is played behind it
FW_TYPES_HD inline void smp_stream_msg(NodeState& s, uint64_t W, int has_end, uint64_t E) {
    if (!smp_stream_on(s)) return;
    SmpStream t = smp_stream_of(s);
    if (W > t.W) t.W = W;
    bool late = false;
    if (has_end && !(t.flags & SMP_STREAM_HAS_END)) {
        t.E = E;
        t.flags |= SMP_STREAM_HAS_END;
        late = t.E <= t.C;
        if (late) t.flags |= SMP_STREAM_FINISHED;
    }
    smp_stream_put(s, t);
    if (late) {
        s.playing = 0;
        smp_env_reset(s);
    }
}
// In front of a block of n frames of a PLAYING sampler, behind the block's messages.  true: the frames are not there (W - C < n) —
// U += 1 and the block is rendered exactly as a block of a sampler that does not play; `playing` itself stays 1
FW_TYPES_HD inline bool smp_stream_starved(NodeState& s, uint32_t n) {
    if (!smp_stream_on(s)) return false;
    SmpStream t = smp_stream_of(s);
    if (t.W - t.C >= (uint64_t)n) return false;
    t.U += 1u;
    smp_stream_put(s, t);
    return true;
}
// How many of a block's n frames lie in front of the end (n: all of them; call it in front of the block's advance).  A block the end
// falls into is rendered as a one-shot's last block — frames from there on are 0.0 (the Fetch's tail_zero) — unless the ring's wrap
// falls in front of the end inside the same block: a record holds one break, so that block reads the padding behind the end from the
// ring (zero bytes; the unsigned 16-bit formats have no element that decodes to 0.0, their padding is 0x8000: 1.5e-5)
FW_TYPES_HD inline uint32_t smp_stream_block_data(const NodeState& s, uint32_t n) {
    if ((smp_stream_flags(s) & (SMP_STREAM_ON | SMP_STREAM_HAS_END)) != (SMP_STREAM_ON | SMP_STREAM_HAS_END)) return n;
    const SmpStream t = smp_stream_of(s);
    if (t.E <= t.C) return 0u;
    return t.E - t.C < (uint64_t)n ? (uint32_t)(t.E - t.C) : n;
}
// CMD_SMP_PAUSE / CMD_SMP_STOP (sampler.rs:372-391), as messages and as what a fade's `then` asks for
FW_TYPES_HD inline void smp_pause(NodeState& s) {
    s.playing = 0;
    smp_env_reset(s);
}
FW_TYPES_HD inline void smp_stop(NodeState& s) {
    if (!smp_stream_on(s)) s.playhead = s.has_loop ? s.loop_start : 0;  // (a stream does not rewind: stop acts as pause)
    s.playing = 0;
    smp_env_reset(s);
}
// Behind a rendered block of n frames (behind smp_env_behind_block); ph0 = the playhead in front of the block.  C moves in exactly
// the blocks in which the playhead moved (a muted voice holds both); at the end the sampler stops where it stands and is finished
FW_TYPES_HD inline void smp_stream_behind_block(NodeState& s, uint64_t ph0, uint32_t n) {
    if (!smp_stream_on(s) || s.playhead == ph0) return;
    SmpStream t = smp_stream_of(s);
    t.C += (uint64_t)n;
    const bool end = (t.flags & SMP_STREAM_HAS_END) && t.C >= t.E;
    if (end) t.flags |= SMP_STREAM_FINISHED;
    smp_stream_put(s, t);
    if (end) smp_pause(s);
}
// behind a rendered block of `frames` frames in which the gain smoother ran (the values are smp_env_value of a snapshot taken BEFORE
// this): k += frames; a fade that is over comes to rest and its `then` takes effect; a sampler that no longer plays — paused or
// stopped by `then`, or a one-shot that ended in this block — has its envelope back at rest at 1.0f
FW_TYPES_HD inline void smp_env_behind_block(NodeState& s, uint32_t frames) {
    const uint32_t N = smp_env_N(s);
    if (N != 0u) {
        const uint32_t k = (uint32_t)s.s1.status + frames;
        if (k < N) {
            s.s1.status = (int)k;
        } else {
            const int then = smp_env_then(s);
            s.enabled = 0;
            s.s1.status = 0;
            if (then == SMP_FADE_PAUSE) smp_pause(s);
            else if (then == SMP_FADE_STOP) smp_stop(s);
        }
    }
    if (!s.playing) smp_env_reset(s);
}
// the sampler's constant gain while its smoother (value c) and its envelope rest: what every frozen / steady / lazy path multiplies by
FW_TYPES_HD inline float smp_rest_gain(const NodeState& s, float c) { return c * s.gain; }

// K_BIQUAD coefficient sweep (SPEC): ONE statement for the message, the node kernels, the control kernel and k_chain's
// sweep instantiation.  The five coefficients (b0 b1 b2 a1 a2) move from A to T over N frames, k of them rendered; at rest (N == 0)
// they are the five at the head of the node's ext slice.  Every operation below is a separately rounded f32 operation
// (-ffp-contract=off), the division is IEEE, and (float)(k + j), (float)N are exact (both <= 2^24).  In the NodeState: s0.status = N,
// s1.status = k, A = s0.{input, last, a, b, eps}, T = s1.{input, last, a, b, eps}
#define BQ_SWEEP_FRAMES_MAX 16777216u
#define BQ_SNAP_LEN 12  // A[5], T[5], N, k as 32-bit words in the float slots
struct BqSweep {
    float A[5], T[5];
    uint32_t N, k;
};
FW_TYPES_HD inline bool bq_sweep_at_rest(const NodeState& s) { return s.s0.status == 0; }
FW_TYPES_HD inline BqSweep bq_sweep_of(const NodeState& s) {
    BqSweep w;
    w.A[0] = s.s0.input, w.A[1] = s.s0.last, w.A[2] = s.s0.a, w.A[3] = s.s0.b, w.A[4] = s.s0.eps;
    w.T[0] = s.s1.input, w.T[1] = s.s1.last, w.T[2] = s.s1.a, w.T[3] = s.s1.b, w.T[4] = s.s1.eps;
    w.N = (uint32_t)s.s0.status;
    w.k = (uint32_t)s.s1.status;
    return w;
}
FW_TYPES_HD inline void bq_sweep_put(NodeState& s, const BqSweep& w) {
    s.s0.input = w.A[0], s.s0.last = w.A[1], s.s0.a = w.A[2], s.s0.b = w.A[3], s.s0.eps = w.A[4];
    s.s1.input = w.T[0], s.s1.last = w.T[1], s.s1.a = w.T[2], s.s1.b = w.T[3], s.s1.eps = w.T[4];
    s.s0.status = (int)w.N;
    s.s1.status = (int)w.k;
}
// the sweep's position j frames ahead, (float)(k + j) / (float)N — one division serves a frame's five coefficients; only for k + j < N
FW_TYPES_HD inline float bq_sweep_pos(const BqSweep& w, uint32_t j) { return (float)(w.k + j) / (float)w.N; }
// c_i(j): coefficient i (a compile-time index wherever a kernel calls this) of the frame j frames ahead; `rest` = the ext head's value
FW_TYPES_HD inline float bq_sweep_coef(const BqSweep& w, int i, uint32_t j, float rest) {
    if (w.N == 0u) return rest;
    if (w.k + j >= w.N) return w.T[i];
    return fw_ramp_mix(w.A[i], w.T[i], w.T[i] - w.A[i], bq_sweep_pos(w, j));
}
// the message, applied at a block's first frame: N frames from where the coefficients stand (head: the ext slice's five) to T.
// frames == 0 is a step: the caller writes T to the ext head (CMD_SET_COEFS does the same); so is frames > BQ_SWEEP_FRAMES_MAX, which
// is NOT SPEC behaviour (fwgpu_biquad_sweep refuses such a call: only a corrupted message gets here).  true: the head must be set to T
FW_TYPES_HD inline bool bq_sweep_start(BqSweep& w, const float head[5], const float T[5], uint32_t frames) {
    float from[5];
    for (int i = 0; i < 5; ++i) from[i] = bq_sweep_coef(w, i, 0u, head[i]);  // a retarget in mid-sweep continues from where the sweep stands
    for (int i = 0; i < 5; ++i) w.T[i] = T[i];
    w.k = 0u;
    if (frames == 0u || frames > BQ_SWEEP_FRAMES_MAX) {
        w.N = 0u;
        return true;
    }
    for (int i = 0; i < 5; ++i) w.A[i] = from[i];
    w.N = frames;
    return false;
}
FW_TYPES_HD inline void bq_sweep_stop(BqSweep& w) { w.N = w.k = 0u; }  // CMD_SET_COEFS: the sweep ends, the message's five are the head
// behind a rendered block of `frames` frames (the values are bq_sweep_coef of the state BEFORE this).  true: the sweep is over — the
// node is at rest again and the caller writes T to the ext head
FW_TYPES_HD inline bool bq_sweep_advance(BqSweep& w, uint32_t frames) {
    if (w.N == 0u) return false;
    const uint32_t k = w.k + frames;  // (k < N <= 2^24 and a block has fewer than 2^31 frames)
    if (k < w.N) {
        w.k = k;
        return false;
    }
    w.N = w.k = 0u;
    return true;
}

// K_SPATIAL move (SPEC): ONE statement for the message (apply_cmds_from), the node kernels, the control kernel and the
// leaf kernel.  Per ear e the gain goes G0 -> G1 over N frames in smp_env_value's form — every operation a separately rounded f32
// operation (-ffp-contract=off), the division IEEE, (float)(k + j) and (float)N exact (both <= 2^24) — and the delay is a 32.32
// unsigned number D that moves by a signed inc per frame, in wrapping u64 arithmetic (the resampler glide's rule: inc is truncated
// toward zero, so D stays between its start and d1 << 32, both <= 63 << 32, and the move's last frame is followed by exactly
// d1 << 32).  A frame reads the mono row at i - (D >> 32) and, when the fraction's top 24 bits are not all zero, blends in the frame
// before it: at rest the fraction is zero and the output bits are the integer delay's.
#define SP_MOVE_FRAMES_MAX 16777216u
struct SpMove {
    float G0[2], G1[2];
    uint64_t D[2], inc[2];  // D: at the snapshot's first frame
    uint32_t d1[2];
    uint32_t N, k;
};
FW_TYPES_HD inline bool sp_move_at_rest(const NodeState& s) { return s.full_range == 0; }
FW_TYPES_HD inline uint32_t sp_delay_ok(int d) { return d < 0 ? 0u : (d > SP_HIST - 1 ? (uint32_t)(SP_HIST - 1) : (uint32_t)d); }
// the move as a block's render loop reads it: a snapshot taken BEFORE the block's advance (at rest: N == 0, D = the integer delays)
FW_TYPES_HD inline SpMove sp_move_of(const NodeState& s) {
    SpMove m;
    m.N = (uint32_t)s.full_range;
    m.k = (uint32_t)s.enabled;
    m.G0[0] = s.phasor, m.G0[1] = s.phasor_inc;
    m.G1[0] = s.p0, m.G1[1] = s.p1;
    m.d1[0] = sp_delay_ok(s.playing), m.d1[1] = sp_delay_ok(s.has_loop);
    if (m.N != 0u) {
        m.D[0] = s.playhead, m.D[1] = s.loop_start;
        m.inc[0] = s.loop_end;
        m.inc[1] = (uint64_t)(uint32_t)s.sample | ((uint64_t)fw_bits_of(s.gain) << 32);
    } else {
        m.D[0] = (uint64_t)m.d1[0] << 32, m.D[1] = (uint64_t)m.d1[1] << 32;
        m.inc[0] = m.inc[1] = 0ull;
    }
    return m;
}
// the gain of ear e, j frames ahead of the snapshot; behind the move, and at rest: G1
FW_TYPES_HD inline float sp_move_gain(const SpMove& m, int e, uint32_t j) {
    const uint32_t t = m.k + j;
    if (t >= m.N) return m.G1[e];
    return fw_ramp_mix(m.G0[e], m.G1[e], m.G1[e] - m.G0[e], (float)t / (float)m.N);
}
// the 32.32 delay of ear e, j frames ahead of the snapshot; behind the move exactly d1 << 32
FW_TYPES_HD inline uint64_t sp_move_delay(const SpMove& m, int e, uint32_t j) {
    return m.k + j >= m.N ? (uint64_t)m.d1[e] << 32 : m.D[e] + (uint64_t)j * m.inc[e];
}
// a delay's whole frames q and its fraction f (24 bits: exact in f32); f != 0 implies q <= 62, so q + 1 stays inside SP_HIST
FW_TYPES_HD inline uint32_t sp_move_whole(uint64_t D) { return (uint32_t)(D >> 32); }
FW_TYPES_HD inline float sp_move_frac(uint64_t D) { return (float)((uint32_t)D >> 8) * 5.9604644775390625e-08f; }
// the same two as ONE 32-bit word per frame and ear — q in bits 24..29, the fraction's 24 bits below — which is how a voice bank's
// control kernel hands a move block's delays to the leaf kernel: in the two rows behind the block's gain rows (FusedView::ramps)
FW_TYPES_HD inline uint32_t sp_move_word(uint64_t D) { return (uint32_t)(D >> 8); }
FW_TYPES_HD inline uint32_t sp_word_whole(uint32_t w) { return w >> 24; }
FW_TYPES_HD inline float sp_word_frac(uint32_t w) { return (float)(w & 0xffffffu) * 5.9604644775390625e-08f; }
// the frame: a = m[i - q], b = m[i - q - 1] (read only where f != 0)
FW_TYPES_HD inline float sp_move_tap(float a, float b, float f) { return f == 0.0f ? a : a + ((b - a) * f); }
// CMD_SET_P0 / _P1 / CMD_SP_ITD in a move (a plain set_position): the move ends — each smoother continues from the move's current
// gain towards whatever the message sets, the delays step to the move's target until a CMD_SP_ITD says otherwise
FW_TYPES_HD inline void sp_move_stop(NodeState& s) {
    if (s.full_range == 0) return;
    const SpMove m = sp_move_of(s);
    s.s0.last = sp_move_gain(m, 0, 0u);
    s.s1.last = sp_move_gain(m, 1, 0u);
    s.full_range = 0;
    s.enabled = 0;
}
// the message, applied at a block's first frame: N frames from where the node stands to (G1l, G1r, d1l, d1r)
FW_TYPES_HD inline void sp_move_start(NodeState& s, float G1l, float G1r, int d1l, int d1r, uint32_t N) {
    const SpMove m = sp_move_of(s);
    const float G0l = m.N ? sp_move_gain(m, 0, 0u) : (s.s0.status == SM_ACTIVE ? s.s0.last : s.s0.input);
    const float G0r = m.N ? sp_move_gain(m, 1, 0u) : (s.s1.status == SM_ACTIVE ? s.s1.last : s.s1.input);
    // the smoothers are put at rest at the target (coefficients untouched)
    s.p0 = s.s0.input = s.s0.last = G1l;
    s.p1 = s.s1.input = s.s1.last = G1r;
    s.s0.status = s.s1.status = SM_INACTIVE;
    const uint32_t tl = sp_delay_ok(d1l), tr = sp_delay_ok(d1r);
    s.playing = (int)tl;
    s.has_loop = (int)tr;
    s.enabled = 0;
    // (N == 0 or N > SP_MOVE_FRAMES_MAX is NOT SPEC behaviour: fwgpu_spatial_move sends the step's own three messages for the first
    //  and refuses the second, so only a corrupted message gets here — a defensive branch, a step)
    if (N == 0u || N > SP_MOVE_FRAMES_MAX) {
        s.full_range = 0;
        return;
    }
    const uint64_t il = fw_glide_inc(m.D[0], (uint64_t)tl << 32, N), ir = fw_glide_inc(m.D[1], (uint64_t)tr << 32, N);
    s.phasor = G0l;
    s.phasor_inc = G0r;
    s.playhead = m.D[0];
    s.loop_start = m.D[1];
    s.loop_end = il;
    s.sample = (int)(uint32_t)ir;
    s.gain = fw_float_of((uint32_t)(ir >> 32));
    s.full_range = (int)N;
}
// behind a rendered block of `frames` frames (the values are sp_move_gain / sp_move_delay of a snapshot taken BEFORE this)
FW_TYPES_HD inline void sp_move_advance(NodeState& s, uint32_t frames) {
    const uint32_t N = (uint32_t)s.full_range;
    if (N == 0u) return;
    const uint32_t k = (uint32_t)s.enabled + frames;  // (k < N <= 2^24 and a block has fewer than 2^31 frames)
    if (k < N) {
        s.enabled = (int)k;
        s.playhead += (uint64_t)frames * s.loop_end;
        s.loop_start += (uint64_t)frames * ((uint64_t)(uint32_t)s.sample | ((uint64_t)fw_bits_of(s.gain) << 32));
    } else {  // at rest: a spatialiser set to the target whose smoothers have settled
        s.full_range = 0;
        s.enabled = 0;
    }
}

// The automation curve y(u) of the crossfader (SPEC) and of a gain ride: ONE statement for xf_positions (k_common.hip.h)
// and gain_ride_value.  Shape 0: y = u.  Shape 1: y = 0 at u == 0, else XF_ITERS bisection steps on B(t; x1, x2) < u, then B(t; y1, y2),
// with B(t; a, d) = ((q*t + b)*t + c)*t, the cubic Bezier coordinate through 0, a, d, 1.  Every operation is a separately rounded f32
// operation (-ffp-contract=off).  The solver runs on W frames at once, its loop rolled: the same trip count for every frame, nothing
// indexed by a variable.  Always inlined: the crossfader's kernels keep the code they had when the solver stood inside xf_positions
#if defined(__HIPCC__)
#define FW_TYPES_UNROLL _Pragma("unroll")
#define FW_TYPES_ROLLED _Pragma("unroll 1")
#else
#define FW_TYPES_UNROLL
#define FW_TYPES_ROLLED
#endif
struct XfCubic {
    float q, b, c;
};
FW_TYPES_HD_INLINE XfCubic xf_cubic(float a, float d) {
    const float c = 3.0f * a;
    const float b = (3.0f * (d - a)) - c;
    return XfCubic{(1.0f - c) - b, b, c};
}
FW_TYPES_HD_INLINE float xf_bezier(const XfCubic& k, float t) { return (((k.q * t) + k.b) * t + k.c) * t; }
template <int W>
FW_TYPES_HD_INLINE void fw_curve_y(int shape, float x1, float y1, float x2, float y2, const float (&u)[W], float (&y)[W]) {
    FW_TYPES_UNROLL
    for (int e = 0; e < W; ++e) y[e] = u[e];
    if (shape == XF_SHAPE_BEZIER) {
        const XfCubic kx = xf_cubic(x1, x2), ky = xf_cubic(y1, y2);
        float lo[W], hi[W];
        FW_TYPES_UNROLL
        for (int e = 0; e < W; ++e) lo[e] = 0.0f, hi[e] = 1.0f;
        FW_TYPES_ROLLED
        for (int i = 0; i < XF_ITERS; ++i) {
            FW_TYPES_UNROLL
            for (int e = 0; e < W; ++e) {
                const float m = (lo[e] + hi[e]) * 0.5f;
                const bool below = xf_bezier(kx, m) < u[e];
                lo[e] = below ? m : lo[e];
                hi[e] = below ? hi[e] : m;
            }
        }
        FW_TYPES_UNROLL
        for (int e = 0; e < W; ++e) y[e] = u[e] == 0.0f ? 0.0f : xf_bezier(ky, (lo[e] + hi[e]) * 0.5f);
    }
}

// K_VOLUME / K_PAN gain ride (SPEC): ONE statement for the message (apply_cmds_from), the node kernels, the control
// kernel and the host.  Per gain c (a volume: c = 0 alone; a pan: the left and the right ear) the gain goes G0_c -> G1_c over N frames
// along the curve y: every operation a separately rounded f32 operation (-ffp-contract=off), the division IEEE, (float)(k + j) and
// (float)N exact (both <= 2^24).  The layout is NodeState's comment block's (VOLUME, PAN); G1 = p0 / p1
#define GAIN_RIDE_FRAMES_MAX 16777216u
struct GainRide {
    float G0[2], G1[2], d[2];  // d = G1 - G0, computed once
    float x1, y1, x2, y2;
    uint32_t N, k;
    int shape;
};
FW_TYPES_HD_INLINE bool gain_ride_at_rest(const NodeState& s) { return s.full_range == 0; }
// the ride as a block's render loop reads it: a snapshot taken BEFORE the block's advance (at rest: N == 0, every value is G1)
FW_TYPES_HD_INLINE GainRide gain_ride_of(const NodeState& s) {
    GainRide r;
    r.N = (uint32_t)s.full_range;
    r.k = (uint32_t)s.enabled;
    r.shape = s.has_loop;
    r.G0[0] = s.phasor, r.G0[1] = s.phasor_inc;
    r.G1[0] = s.p0, r.G1[1] = s.p1;
    r.d[0] = r.G1[0] - r.G0[0], r.d[1] = r.G1[1] - r.G0[1];
    r.x1 = fw_float_of((uint32_t)s.playhead), r.y1 = fw_float_of((uint32_t)(s.playhead >> 32));
    r.x2 = fw_float_of((uint32_t)s.loop_start), r.y2 = fw_float_of((uint32_t)(s.loop_start >> 32));
    return r;
}
// ride_c(j) .. ride_c(j + W - 1), the gains of W consecutive frames from j frames ahead of the snapshot: behind the ride, and at rest,
// G1; fw_ramp_mix's clamp keeps an overshooting curve inside [min(G0, G1), max(G0, G1)]
template <int W>
FW_TYPES_HD_INLINE void gain_ride_values(const GainRide& r, int c, uint32_t j, float (&g)[W]) {
    FW_TYPES_UNROLL
    for (int e = 0; e < W; ++e) g[e] = r.G1[c];
    const uint64_t t0 = (uint64_t)r.k + (uint64_t)j;
    if (r.N == 0u || t0 >= (uint64_t)r.N) return;
    const float fN = (float)r.N;
    float u[W], y[W];
    FW_TYPES_UNROLL
    for (int e = 0; e < W; ++e) u[e] = (float)((uint32_t)t0 + (uint32_t)e) / fN;
    fw_curve_y<W>(r.shape, r.x1, r.y1, r.x2, r.y2, u, y);
    FW_TYPES_UNROLL
    for (int e = 0; e < W; ++e)
        if (t0 + (uint64_t)e < (uint64_t)r.N) g[e] = fw_ramp_mix(r.G0[c], r.G1[c], r.d[c], y[e]);  // (the ride may end among the W frames)
}
FW_TYPES_HD inline float gain_ride_value(const GainRide& r, int c, uint32_t j) {
    float g[1];
    gain_ride_values<1>(r, c, j, g);
    return g[0];
}
// param 0 in a ride (CMD_SET_P0 / _P1): the ride ends — each smoother is reset to the ride's current gain and continues from there
// towards whatever the message sets
FW_TYPES_HD inline void gain_ride_clear(NodeState& s) {  // at rest: every field of the ride as make_state leaves it
    s.full_range = 0;
    s.enabled = 0;
    s.has_loop = 0;
    s.phasor = s.phasor_inc = 0.0f;
    s.playhead = s.loop_start = 0ull;
}
FW_TYPES_HD inline void gain_ride_end(NodeState& s) {
    if (s.full_range == 0) return;
    const GainRide r = gain_ride_of(s);
    s.s0.input = s.s0.last = gain_ride_value(r, 0, 0u);
    s.s1.input = s.s1.last = gain_ride_value(r, 1, 0u);
    s.s0.status = s.s1.status = SM_INACTIVE;
    gain_ride_clear(s);
}
// the message, applied at a block's first frame: N frames from where the node stands to (G1_0, G1_1) along the curve.  N == 0 is the
// SPEC's step: the gains are set hard, with no glide of the smoothers
FW_TYPES_HD inline void gain_ride_start(NodeState& s, float G1_0, float G1_1, uint32_t N, int shape, float x1, float y1, float x2, float y2) {
    const GainRide r = gain_ride_of(s);
    const float G0_0 = r.N ? gain_ride_value(r, 0, 0u) : (s.s0.status == SM_ACTIVE ? s.s0.last : s.s0.input);
    const float G0_1 = r.N ? gain_ride_value(r, 1, 0u) : (s.s1.status == SM_ACTIVE ? s.s1.last : s.s1.input);
    // the smoothers are put at rest at the targets (coefficients untouched)
    s.p0 = s.s0.input = s.s0.last = G1_0;
    s.p1 = s.s1.input = s.s1.last = G1_1;
    s.s0.status = s.s1.status = SM_INACTIVE;
    gain_ride_clear(s);
    // (N > GAIN_RIDE_FRAMES_MAX or a shape outside 0..1 is NOT SPEC behaviour: fwgpu_gain_ride refuses such a call, so only a
    //  corrupted message gets here — a defensive branch, a step)
    if (N == 0u || N > GAIN_RIDE_FRAMES_MAX || (shape != XF_SHAPE_LINEAR && shape != XF_SHAPE_BEZIER)) return;
    s.phasor = G0_0;
    s.phasor_inc = G0_1;
    s.has_loop = shape;
    s.playhead = (uint64_t)fw_bits_of(x1) | ((uint64_t)fw_bits_of(y1) << 32);
    s.loop_start = (uint64_t)fw_bits_of(x2) | ((uint64_t)fw_bits_of(y2) << 32);
    s.full_range = (int)N;
}
// behind a block of `frames` frames the node was processed in, silent input or not (the values are gain_ride_value of a snapshot
// taken BEFORE this)
FW_TYPES_HD inline void gain_ride_behind_block(NodeState& s, uint32_t frames) {
    const uint32_t N = (uint32_t)s.full_range;
    if (N == 0u) return;
    const uint32_t k = (uint32_t)s.enabled + frames;  // (k < N <= 2^24 and a block has fewer than 2^31 frames)
    if (k < N) {
        s.enabled = (int)k;
    } else {  // at rest: a node set to the target whose smoother has settled
        gain_ride_clear(s);
    }
}

// K_CROSSFADE (rendered by k_level<0>, no ext slice): the states its case renders.  T never runs behind t0: a message sets t0 = T
FW_TYPES_HD inline bool xf_state_ok(const NodeState& s, int n_in, int n_out) {
    const auto unit = [](float x) { return x >= 0.0f && x <= 1.0f; };  // (false for a NaN)
    const auto ctl_y = [](float y) { return y >= -1.0f && y <= 2.0f; };
    return s.loop_end == 1 && n_out >= 1 && n_out <= XF_CH_MAX && n_in == 2 * n_out && unit(s.p0) && unit(s.p1) && s.full_range >= 0 &&
           (uint32_t)s.full_range <= XF_FRAMES_MAX && (s.has_loop == XF_SHAPE_LINEAR || s.has_loop == XF_SHAPE_BEZIER) &&
           (s.playing == XF_LAW_LINEAR || s.playing == XF_LAW_EQUAL_POWER) && unit(s.phasor) && unit(s.gain) && ctl_y(s.phasor_inc) &&
           ctl_y(s.aux) && s.playhead >= s.loop_start;
}
// The crossfader's position rule (SPEC): ONE statement for the crossfader's message and render case (k_common.hip.h,
// k_generic.hip.h), the FIR morph (fir_morph_* below) and a host build.  The segment as the rule reads it:
struct XfSeg {
    float P0, P1, x1, y1, x2, y2;
    uint64_t t0;
    uint32_t dur;
    int shape;
};
FW_TYPES_HD_INLINE XfSeg xf_seg(const NodeState& s) {
    return XfSeg{s.p0, s.p1, s.phasor, s.phasor_inc, s.gain, s.aux, s.loop_start, (uint32_t)s.full_range, s.has_loop};
}
// the positions of frames n .. n + W - 1 (node time) under the segment.  The solver — XF_ITERS bisection steps on x(t) = u, then
// y(t) — runs on the W frames at once, its loop rolled: the same trip count for every frame, nothing indexed by a variable
template <int W>
FW_TYPES_HD_INLINE void xf_positions(const XfSeg& g, uint64_t n, float (&p)[W]) {
    const uint32_t dur = g.dur;
    const uint64_t k0 = n - g.t0;
    FW_TYPES_UNROLL
    for (int e = 0; e < W; ++e) p[e] = g.P1;
    if (dur == 0u || k0 >= (uint64_t)dur) return;
    const float fdur = (float)dur;  // (exact: dur <= 2^24; so is every k < dur)
    float u[W], y[W];
    FW_TYPES_UNROLL
    for (int e = 0; e < W; ++e) u[e] = (float)((uint32_t)k0 + (uint32_t)e) / fdur;
    fw_curve_y<W>(g.shape, g.x1, g.y1, g.x2, g.y2, u, y);
    const float span = g.P1 - g.P0;
    FW_TYPES_UNROLL
    for (int e = 0; e < W; ++e)
        if (k0 + (uint64_t)e < (uint64_t)dur)  // (the segment may end among the W frames)
            p[e] = fminf(fmaxf(g.P0 + (span * y[e]), 0.0f), 1.0f);  // an overshooting curve is allowed; the position is clamped
}
FW_TYPES_HD_INLINE void xf_gains(int law, float p, float& a, float& b) {
    const float q = 1.0f - p;
    a = law == XF_LAW_LINEAR ? q : sqrtf(q);
    b = law == XF_LAW_LINEAR ? p : sqrtf(p);
}

struct SampleDesc {  // core/sample_resource.rs:4-26; data is HBM-resident
    const void* data;
    uint64_t frames;
    int channels;
    int format;
};

// Static description of one scheduled node (graph/graph/compiler/schedule.rs:12-20 after buffer renaming).
struct NodeDesc {
    int kind;
    int n_in, n_out;
    int in_off, out_off;  // offsets into the port tables
    int state;            // NodeState index
    int aux0;             // SUM: num_in_ports (low 16 bits); high 16 bits, when set: the port count whose path the node takes
                          //      (sum.rs:67-133: 2 / 3 / 4 ports add unmasked, any other count skips silent ports) — the
                          //      continuation of a SumNode whose leading voice ports were summed by the voice-bank kernels
    int is_graph_io;      // 1 = graph_in, 2 = graph_out (Dummy nodes the executor treats as I/O edges)
};

// control -> audio messages (nodes/sampler.rs:21-28 + the atomics), sorted by (state, block, seq).
// What a type carries in i0 / f0 / i1 / d0 / d1 is stated ONCE, by its maker below the struct (make_*); nothing else writes those
// fields, and what is not a single plain field is read through the reader beside the maker.
enum : int {
    CMD_SET_P0 = 0, CMD_SET_P1 = 1, CMD_SET_ENABLED = 2, CMD_SET_GAIN = 3,
    CMD_SET_COEFS = 4,
    CMD_SMP_SET_SAMPLE = 10, CMD_SMP_PLAY = 11, CMD_SMP_PAUSE = 12, CMD_SMP_STOP = 13,
    CMD_SMP_SET_PLAYHEAD = 14, CMD_SMP_SET_LOOP = 15,
    CMD_SMP_FADE = 16,
    CMD_SMP_STREAM = 17,
    CMD_RS_STEP = 20,
    CMD_RS_SEEK = 21,
    CMD_SP_ITD = 22,
    CMD_XF_TO = 23,
    CMD_RS_GLIDE = 24,
    CMD_BQ_SWEEP = 25,
    CMD_SP_MOVE = 26,
    CMD_GAIN_RIDE = 27,
};
struct Cmd {
    int state;
    uint32_t block;
    int type;
    int i0;
    float f0;
    int i1;
    double d0, d1;
};
static_assert(sizeof(Cmd) == 40, "Cmd layout");
// ---- the wire format: one maker per message type, one reader per payload that is not a single plain field.  A maker returns the
// whole message but `state`, which push_cmd fills in (the struct has no padding: Cmd{} leaves every bit it does not set 0).
// The readers are macros over a Cmd lvalue `c`, not functions: a kernel's loop holds its message in a local copy, and a copy whose
// address goes to a function is split into scalars only after inlining — the control kernel then came out with 32 more bytes of
// scratch per lane and 1.3 % slower under a sweep.  As macros they are the field reads they replace, for the compiler too.
FW_TYPES_HD constexpr Cmd make_cmd(int type, uint32_t block) {
    Cmd m{};
    m.type = type;
    m.block = block;
    return m;
}
// CMD_SET_P0 / _P1 / _GAIN: f0 = the value
FW_TYPES_HD constexpr Cmd make_set(int type, uint32_t block, float value) {
    Cmd m = make_cmd(type, block);
    m.f0 = value;
    return m;
}
// CMD_SET_ENABLED: i0 = 0 / 1
FW_TYPES_HD constexpr Cmd make_set_enabled(uint32_t block, bool on) {
    Cmd m = make_cmd(CMD_SET_ENABLED, block);
    m.i0 = on ? 1 : 0;
    return m;
}
// CMD_SET_COEFS (frames == 0) / CMD_BQ_SWEEP (bq_sweep_start), biquad: b0 in f0, b1 and b2 as float bits in i0 and i1, (a1, a2) as
// a pair in d0, d1 bits = the frames to reach them over
FW_TYPES_HD constexpr Cmd make_bq_coefs(uint32_t block, const float co[5], uint32_t frames) {
    Cmd m = make_cmd(frames ? CMD_BQ_SWEEP : CMD_SET_COEFS, block);
    m.f0 = co[0];
    m.i0 = (int)fw_bits_of(co[1]);
    m.i1 = (int)fw_bits_of(co[2]);
    m.d0 = fw_double_of2(co[3], co[4]);
    m.d1 = fw_double_of((uint64_t)frames);
    return m;
}
FW_TYPES_HD constexpr void bq_coefs_of_fields(float f0, int i0, int i1, double d0, float co[5]) {
    co[0] = f0;
    co[1] = fw_float_of((uint32_t)i0);
    co[2] = fw_float_of((uint32_t)i1);
    co[3] = fw_lo_float_of(d0);
    co[4] = fw_hi_float_of(d0);
}
#define bq_cmd_coefs(c, co) fwgpu::bq_coefs_of_fields((c).f0, (c).i0, (c).i1, (c).d0, (co))
#define bq_cmd_frames(c) ((uint32_t)fwgpu::fw_bits_of64((c).d1))
// CMD_SMP_SET_SAMPLE: i0 = the sample id, i1 = stop_playback; of a stream (smp_stream_bind), d0 bits = R, the ring's frames (0: no
// stream), d1 bits = W, the frames written so far
FW_TYPES_HD constexpr Cmd make_smp_set_sample(uint32_t block, int sample, bool stop, uint64_t R, uint64_t W) {
    Cmd m = make_cmd(CMD_SMP_SET_SAMPLE, block);
    m.i0 = sample;
    m.i1 = stop ? 1 : 0;
    m.d0 = fw_double_of(R);
    m.d1 = fw_double_of(W);
    return m;
}
#define smp_cmd_sample(c) ((c).i0)
#define smp_cmd_stop(c) ((c).i1 != 0)
#define smp_cmd_ring(c) (fwgpu::fw_bits_of64((c).d0))
#define smp_cmd_written(c) (fwgpu::fw_bits_of64((c).d1))
// CMD_SMP_PLAY / _PAUSE / _STOP (a resampling source takes play and pause too): no payload
FW_TYPES_HD constexpr Cmd make_smp_transport(int type, uint32_t block) { return make_cmd(type, block); }
// CMD_SMP_FADE (smp_env_start): f0 = the target gain (0..1), i0 = the frames to reach it over, i1 = then (SMP_FADE_*)
FW_TYPES_HD constexpr Cmd make_smp_fade(uint32_t block, float target, uint32_t frames, int then) {
    Cmd m = make_cmd(CMD_SMP_FADE, block);
    m.f0 = target;
    m.i0 = (int)frames;
    m.i1 = then;
    return m;
}
// CMD_SMP_STREAM (smp_stream_msg), always at block 0: d0 bits = W, the frames written so far; i0 != 0: the stream has ended, d1
// bits = E, its end
FW_TYPES_HD constexpr Cmd make_smp_stream(uint64_t W, bool has_end, uint64_t E) {
    Cmd m = make_cmd(CMD_SMP_STREAM, 0u);
    m.i0 = has_end ? 1 : 0;
    m.d0 = fw_double_of(W);
    m.d1 = fw_double_of(E);
    return m;
}
#define smp_cmd_stream_written(c) (fwgpu::fw_bits_of64((c).d0))
#define smp_cmd_stream_has_end(c) ((c).i0)
#define smp_cmd_stream_end(c) (fwgpu::fw_bits_of64((c).d1))
// CMD_SMP_SET_PLAYHEAD: d0 = seconds
FW_TYPES_HD constexpr Cmd make_smp_set_playhead(uint32_t block, double secs) {
    Cmd m = make_cmd(CMD_SMP_SET_PLAYHEAD, block);
    m.d0 = secs;
    return m;
}
#define smp_cmd_playhead_secs(c) ((c).d0)
// CMD_SMP_SET_LOOP: i0 = mode (0 off, 1 the whole sample, 2 a range), d0 / d1 = the range's start / end in seconds
FW_TYPES_HD constexpr Cmd make_smp_set_loop(uint32_t block, int mode, double start, double end) {
    Cmd m = make_cmd(CMD_SMP_SET_LOOP, block);
    m.i0 = mode;
    m.d0 = start;
    m.d1 = end;
    return m;
}
#define smp_cmd_loop_start_secs(c) ((c).d0)
#define smp_cmd_loop_end_secs(c) ((c).d1)
// CMD_RS_STEP (frames == 0) / CMD_RS_GLIDE (rs_glide_start), resampler: d0 bits = the u64 32.32 step, i0 = the frames to reach it over
FW_TYPES_HD constexpr Cmd make_rs_step(uint32_t block, uint64_t step, uint32_t frames) {
    Cmd m = make_cmd(frames ? CMD_RS_GLIDE : CMD_RS_STEP, block);
    m.i0 = (int)frames;
    m.d0 = fw_double_of(step);
    return m;
}
#define rs_cmd_step(c) (fwgpu::fw_bits_of64((c).d0))
// CMD_RS_SEEK, resampler: d0 bits = the u64 source frame
FW_TYPES_HD constexpr Cmd make_rs_seek(uint32_t block, uint64_t frame) {
    Cmd m = make_cmd(CMD_RS_SEEK, block);
    m.d0 = fw_double_of(frame);
    return m;
}
#define rs_cmd_frame(c) (fwgpu::fw_bits_of64((c).d0))
// CMD_SP_ITD, spatialiser: i0 / i1 = the left / right ear's delay in frames.  f0 = the right ear's gain, which the CMD_SET_P1 in front
// of it delivers: nothing reads it here — the first encoder left it in the record, and the wire pin (tests/test_cmd_wire.py) keeps it
FW_TYPES_HD constexpr Cmd make_sp_itd(uint32_t block, float gr, int dl, int dr) {
    Cmd m = make_cmd(CMD_SP_ITD, block);
    m.f0 = gr;
    m.i0 = dl;
    m.i1 = dr;
    return m;
}
// CMD_SP_MOVE (sp_move_start), spatialiser: (G1l, G1r), the target ear gains, as a pair in d0; i0 = the target delays, the left
// ear's in bits 0..5 and the right ear's in bits 6..11; i1 = the frames to reach them over
FW_TYPES_HD constexpr Cmd make_sp_move(uint32_t block, float gl, float gr, int dl, int dr, uint32_t frames) {
    Cmd m = make_cmd(CMD_SP_MOVE, block);
    m.i0 = (dl & 63) | ((dr & 63) << 6);
    m.i1 = (int)frames;
    m.d0 = fw_double_of2(gl, gr);
    return m;
}
#define sp_cmd_gl(c) (fwgpu::fw_lo_float_of((c).d0))
#define sp_cmd_gr(c) (fwgpu::fw_hi_float_of((c).d0))
#define sp_cmd_dl(c) ((c).i0 & 63)
#define sp_cmd_dr(c) (((c).i0 >> 6) & 63)
#define sp_cmd_frames(c) ((uint32_t)(c).i1)
// CMD_XF_TO, crossfader: f0 = the target position, i0 = frames, i1 = shape (XF_SHAPE_*), the Bezier's control values as pairs:
// (x1, y1) in d0, (x2, y2) in d1
FW_TYPES_HD constexpr Cmd make_xf_to(uint32_t block, float position, uint32_t frames, int shape, float x1, float y1, float x2, float y2) {
    Cmd m = make_cmd(CMD_XF_TO, block);
    m.f0 = position;
    m.i0 = (int)frames;
    m.i1 = shape;
    m.d0 = fw_double_of2(x1, y1);
    m.d1 = fw_double_of2(x2, y2);
    return m;
}
#define xf_cmd_x1(c) (fwgpu::fw_lo_float_of((c).d0))
#define xf_cmd_y1(c) (fwgpu::fw_hi_float_of((c).d0))
#define xf_cmd_x2(c) (fwgpu::fw_lo_float_of((c).d1))
#define xf_cmd_y2(c) (fwgpu::fw_hi_float_of((c).d1))
// CMD_GAIN_RIDE (gain_ride_start), volume / pan: i0 = the frames in bits 0..24 and the shape (XF_SHAPE_*) in bit 28, f0 = G1_0, i1 =
// G1_1 as float bits (a volume: 0.0f), the Bezier's control values as CMD_XF_TO carries them (the xf_cmd_* readers)
FW_TYPES_HD constexpr Cmd make_gain_ride(uint32_t block, float g0, float g1, uint32_t frames, int shape, float x1, float y1, float x2, float y2) {
    Cmd m = make_cmd(CMD_GAIN_RIDE, block);
    m.i0 = (int)((frames & 0x1ffffffu) | ((uint32_t)(shape & 1) << 28));
    m.f0 = g0;
    m.i1 = (int)fw_bits_of(g1);
    m.d0 = fw_double_of2(x1, y1);
    m.d1 = fw_double_of2(x2, y2);
    return m;
}
#define gr_cmd_frames(c) ((uint32_t)(c).i0 & 0x1ffffffu)
#define gr_cmd_shape(c) (((c).i0 >> 28) & 1)
#define gr_cmd_g0(c) ((c).f0)
#define gr_cmd_g1(c) (fwgpu::fw_float_of((uint32_t)(c).i1))
// Round trips, maker to reader, in every build: payload bits that read as a NaN or an infinity when viewed as a double or a float
// (0x7ff0000000000001 is a signalling NaN, 0x7fa00001 too) and -0.0f come back as they went in.
namespace wire_check {
constexpr uint64_t SNAN64 = 0x7ff0000000000001ull, INF64 = 0x7ff0000000000000ull, ALL64 = ~0ull;
constexpr uint32_t SNAN32 = 0x7fa00001u, NEG0 = 0x80000000u;
constexpr bool bq(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t a1, uint32_t a2, uint32_t frames) {
    const float co[5] = {fw_float_of(b0), fw_float_of(b1), fw_float_of(b2), fw_float_of(a1), fw_float_of(a2)};
    const Cmd m = make_bq_coefs(7u, co, frames);
    float r[5] = {};
    bq_cmd_coefs(m, r);
    return m.type == (frames ? CMD_BQ_SWEEP : CMD_SET_COEFS) && m.block == 7u && m.state == 0 && bq_cmd_frames(m) == frames &&
           fw_bits_of(r[0]) == b0 && fw_bits_of(r[1]) == b1 && fw_bits_of(r[2]) == b2 && fw_bits_of(r[3]) == a1 && fw_bits_of(r[4]) == a2;
}
static_assert(bq(NEG0, SNAN32, 0x3f800000u, 0xffffffffu, NEG0, 0u) && bq(SNAN32, NEG0, NEG0, 0x7ff00000u, 0x00000001u, 16777216u) &&
              bq(0u, 0u, 0u, 0x00000001u, 0x7ff00000u, 0xffffffffu), "CMD_SET_COEFS / CMD_BQ_SWEEP");
constexpr bool set_sample(int sample, bool stop, uint64_t R, uint64_t W) {
    const Cmd m = make_smp_set_sample(3u, sample, stop, R, W);
    return m.type == CMD_SMP_SET_SAMPLE && smp_cmd_sample(m) == sample && smp_cmd_stop(m) == stop && smp_cmd_ring(m) == R && smp_cmd_written(m) == W;
}
static_assert(set_sample(5, true, SNAN64, INF64) && set_sample(-1, false, 0ull, ALL64) && set_sample(0x7fffffff, true, 1ull << 33, (1ull << 40) + 1ull),
              "CMD_SMP_SET_SAMPLE");
constexpr bool stream(uint64_t W, bool has_end, uint64_t E) {
    const Cmd m = make_smp_stream(W, has_end, E);
    return m.type == CMD_SMP_STREAM && m.block == 0u && smp_cmd_stream_written(m) == W && (smp_cmd_stream_has_end(m) != 0) == has_end &&
           smp_cmd_stream_end(m) == E;
}
static_assert(stream(SNAN64, true, INF64) && stream(ALL64, false, 0ull) && stream((1ull << 32) + 170ull, true, SNAN64), "CMD_SMP_STREAM");
constexpr bool seconds(double a, double b) {
    const Cmd p = make_smp_set_playhead(1u, a), l = make_smp_set_loop(2u, 2, a, b);
    return fw_bits_of64(smp_cmd_playhead_secs(p)) == fw_bits_of64(a) && l.i0 == 2 && fw_bits_of64(smp_cmd_loop_start_secs(l)) == fw_bits_of64(a) &&
           fw_bits_of64(smp_cmd_loop_end_secs(l)) == fw_bits_of64(b);
}
static_assert(seconds(-0.0, 1.75) && seconds(fw_double_of(INF64), fw_double_of(SNAN64)), "CMD_SMP_SET_PLAYHEAD / CMD_SMP_SET_LOOP");
constexpr bool rs(uint64_t u, uint32_t frames) {
    const Cmd m = make_rs_step(9u, u, frames), k = make_rs_seek(9u, u);
    return m.type == (frames ? CMD_RS_GLIDE : CMD_RS_STEP) && (uint32_t)m.i0 == frames && rs_cmd_step(m) == u && k.type == CMD_RS_SEEK && rs_cmd_frame(k) == u;
}
static_assert(rs(SNAN64, 0u) && rs(INF64, 16777216u) && rs(ALL64, 1u) && rs(1ull << 40, 0u), "CMD_RS_STEP / CMD_RS_GLIDE / CMD_RS_SEEK");
constexpr bool xf(uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2) {
    const Cmd m = make_xf_to(4u, 0.25f, 16777216u, XF_SHAPE_BEZIER, fw_float_of(x1), fw_float_of(y1), fw_float_of(x2), fw_float_of(y2));
    return m.type == CMD_XF_TO && m.f0 == 0.25f && m.i0 == 16777216 && m.i1 == XF_SHAPE_BEZIER && fw_bits_of(xf_cmd_x1(m)) == x1 &&
           fw_bits_of(xf_cmd_y1(m)) == y1 && fw_bits_of(xf_cmd_x2(m)) == x2 && fw_bits_of(xf_cmd_y2(m)) == y2;
}
static_assert(xf(NEG0, SNAN32, 0x3f800000u, 0x7ff00000u) && xf(0x7ff00000u, 0x00000001u, SNAN32, NEG0), "CMD_XF_TO");
constexpr bool sp(uint32_t gl, uint32_t gr, int dl, int dr, uint32_t frames) {
    const Cmd m = make_sp_move(6u, fw_float_of(gl), fw_float_of(gr), dl, dr, frames);
    return m.type == CMD_SP_MOVE && m.block == 6u && m.state == 0 && fw_bits_of(sp_cmd_gl(m)) == gl && fw_bits_of(sp_cmd_gr(m)) == gr &&
           sp_cmd_dl(m) == dl && sp_cmd_dr(m) == dr && sp_cmd_frames(m) == frames;
}
static_assert(sp(NEG0, SNAN32, 0, 63, 1u) && sp(0x7ff00000u, 0x00000001u, 63, 0, 16777216u) && sp(0x3f800000u, NEG0, 32, 31, 0xffffffffu), "CMD_SP_MOVE");
constexpr bool gr(uint32_t g0, uint32_t g1, uint32_t frames, int shape, uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2) {
    const Cmd m = make_gain_ride(5u, fw_float_of(g0), fw_float_of(g1), frames, shape, fw_float_of(x1), fw_float_of(y1), fw_float_of(x2), fw_float_of(y2));
    return m.type == CMD_GAIN_RIDE && m.block == 5u && m.state == 0 && fw_bits_of(gr_cmd_g0(m)) == g0 && fw_bits_of(gr_cmd_g1(m)) == g1 &&
           gr_cmd_frames(m) == frames && gr_cmd_shape(m) == shape && fw_bits_of(xf_cmd_x1(m)) == x1 && fw_bits_of(xf_cmd_y1(m)) == y1 &&
           fw_bits_of(xf_cmd_x2(m)) == x2 && fw_bits_of(xf_cmd_y2(m)) == y2;
}
static_assert(gr(NEG0, SNAN32, 0u, 1, 0x3f800000u, 0x7ff00000u, NEG0, SNAN32) && gr(0x7ff00000u, 0x00000001u, 16777216u, 0, SNAN32, NEG0, 0u, 1u) &&
              gr(0x3f800000u, NEG0, 1u, 1, 0x3ed70a3du, 0u, 0x3f147ae1u, 0x3f800000u), "CMD_GAIN_RIDE");
}  // namespace wire_check

// ---------------------------------------------------------------- fused voice-bank plan
#define FW_MAX_STAGES 6    // sampler gain + up to 5 chain nodes (volume / pan / width / hard clip) in any order
#define FW_CHAIN_STAGES 4  // what k_chain keeps in registers: sampler gain + up to 3 gain stages behind the biquad / delay
// what a chain stage does to the voice's two channels (4 bits per stage in FusedView::progs[voice], stage 1 in bits 0..3);
// the stage's values sit in the gain set: g[j][0], g[j][1]
enum : uint32_t {
    SK_GAIN = 0,   // volume / pan:  L *= g0;  R *= g1                                   (volume.rs:123-126)
    SK_WIDTH = 1,  // stereo width:  m = (L+R)*0.5; s = ((L-R)*0.5)*g0;  L = m+s; R = m-s (SPEC)
    SK_CLIP = 2,   // hard clip:     x = max(min(x, g0), -g0) on both channels            (hard_clip.rs:70-76)
    SK_SPATIAL = 3,  // 3D spatialiser (SPEC), LAST stage only: m = (L+R)*0.5; L = m[i-dL]*g0; R = m[i-dR]*g1 with the
                     // per-ear delays of the block's record (VB_SP_SHIFT) and the 64-frame mono history of the block before
};

// static per voice chain.  Voice-bank plan: source -> [volume|pan|width|hard clip|spatialiser]* -> leaf sum port.  Chain plan (round 6
// grammar): sampler -> G* -> F1 [-> G* -> F2 [-> G* -> F3]] -> G* -> leaf sum port, G = volume | pan | hard clip (<= 3 in all), F1 F2 F3 one of
//   biquad, biquad biquad, delay, biquad delay, biquad biquad delay  (fx_order 0: filters first)   or
//   delay biquad, delay biquad biquad                                (fx_order 1: the delay line first)
struct VoiceDesc {
    int sampler_state;
    int n_stages;                      // gain-like stages of the chain, in schedule order: the first n_pre sit between the source and the
    int stage_kind[FW_MAX_STAGES - 1]; //   biquad / delay (they see the source's silence flag), the rest behind them (they never see one)
    int stage_state[FW_MAX_STAGES - 1];
    int bq_state;                      // the (first) biquad of the chain, -1 = none (k_chain plan)
    int dl_state;                      // the delay line, -1 = none
    int src_kind;                      // 0 = SamplerNode, 1 = SPEC resampling source (sampler_state = its state; no gain of its own),
                                       // 2 = a ONE-output SamplerNode behind a MonoToStereoNode: channel 0 on both outputs (round 5)
    int sp_ext_off;                    // a SPEC spatialiser as the last stage: ext-pool offset of its SP_HIST-frame mono history; -1 = none
    int n_pre;                         // chain plan: gain stages in FRONT of the first filter (0 for a dry voice)
    int bq2_state;                     // chain plan: a second biquad behind the first (an EQ cascade), -1 = none
    int fx_order;                      // chain plan: 0 = biquad(s) then delay, 1 = delay then biquad(s)
    int n_mid;                         // chain plan: gain stages BETWEEN the filters: bits 0..7 between the first and the second, 8..15 between
                                       //   the second and the third (the stages behind n_pre, in schedule order)
};
static_assert(sizeof(VoiceDesc) == 80, "VoiceDesc layout");
// Plan adoption: is voice `nv` of the new plan the same chain as voice `ov` of the old one, so that its steady cache may travel
// (k_exchange.hip.h carry_cache_voice; the host harness holds the same function to a statement of its own,
// tests/host_harness/launch_stubs.cpp check_carry)?  The WHOLE descriptor is compared: a steady cache — "silent", the gain set, the
// -1.0 sentinel of a stage muted between two filters — means what it means only for one arrangement of stages around the filters,
// and a list of fields kept by hand had fallen behind the grammar (n_mid: the same nodes with a gain moved across a filter compared
// equal).  The plan build clears a descriptor before it fills it, so unused stage slots compare equal too.
FW_TYPES_HD inline bool same_voice_chain(const VoiceDesc& nv, const VoiceDesc& ov) {
    static_assert(sizeof(VoiceDesc) % sizeof(int) == 0 && alignof(VoiceDesc) == alignof(int), "VoiceDesc: ints only, no padding");
    const int* const a = (const int*)&nv;
    const int* const b = (const int*)&ov;
    bool same = true;
    for (unsigned i = 0; i < sizeof(VoiceDesc) / sizeof(int); ++i) same = same && a[i] == b[i];
    return same;
}

// per (block, voice) record written by the control kernels, read by the leaf kernel (80 B)
enum : uint32_t {
    VB_SILENT = 1u,       // chain output is cleared + flagged silent for this block
    VB_WRAP = 2u,         // loop wrap inside the block: frames [n1, frames) come from off1
    VB_TAIL_ZERO = 4u,    // one-shot end inside the block: frames [n1, frames) are 0.0
    VB_MONO = 8u,         // 1-channel sample duplicated to both outputs (sampler.rs:546-551)
    VB_SIMPLE = 16u,      // contiguous planar-f32 source + constant gains: src_l/src_r valid, fast path
                          //   (k_chain plan: also a VB_SRC_ZERO block with constant gains; no full VoiceBlk either way)
    VB_SRC_ZERO = 32u,    // the sampler's output is cleared this block (differs from VB_SILENT only when a biquad /
                          //   delay sits between the sampler and the gain stages: their tails keep ringing)
    VB_RESAMPLE = 64u,    // resampling source (SPEC): off0 = 32.32 position of frame 0, off1 = 32.32 step, n1 = loops;
                          //   every such block carries a full VoiceBlk (the 16-tap polyphase fetch is the leaf kernel's slow path)
    VB_RS_LEAN = 128u,    // a resampler block of a STEADY voice (VoiceRef::flags_gset only; round 4): its full descriptor is the voice's
                          //   template FusedView::rs_tmpl[voice] — written once per call — with off0 = the 32.32 position carried in
                          //   VoiceRef::src_l; no VoiceBlk row is written for it (they were 75 MB per 768-block call of 1 024 voices,
                          //   and what the control kernel's 42 us went into)
    VB_RS_GLIDE = 1u << 27,  // a VB_RESAMPLE block inside a ratio glide (VoiceBlk::flags only, never lean): the step changes by inc per frame —
                          //   rs_glide_pack / rs_glide_rem above say where inc, left and the target sit; the frame-by-frame fetch renders it
    VB_FMT_SHIFT = 24,    // VB_RESAMPLE blocks: bits 24..26 = the sample's format (FMT_*), src_l = its data, pad = its frames (< 2^31)
                          //   — the leaf kernel needs no second dependent load for the sample table
    VB_RAMP_SHIFT = 8,    // bit (VB_RAMP_SHIFT + 2*stage + ch): that gain is a per-frame ramp (12 bits: 8..19)
    VB_RAMP_MASK = 0xfffu << 8,
    VB_SP_SHIFT = 20,     // voices whose last stage is a spatialiser: bits 20..25 = left-ear delay, 26..31 = right-ear delay (frames,
                          //   <= 63) in force for this block — in VoiceBlk::flags AND VoiceRef::flags_gset (such a voice's source is
                          //   never a resampler, so the VB_FMT bits are free)
    VB_SP_MASK = 0xfffu << 20,
};
struct VoiceBlk {
    uint32_t flags;
    uint32_t n1;         // frames taken from off0 (VB_RESAMPLE: bit 0 = the source loops; VB_RS_GLIDE: rs_glide_rem above it)
    const float* src_l;  // frame 0 of channel 0 / 1 when the block's frames are contiguous planar f32
    const float* src_r;
    uint64_t off0;       // source frame of frame 0
    uint64_t off1;       // source frame of frame n1 when VB_WRAP
    int sample;          // sample-table index
    uint32_t pad;
    float g[FW_MAX_STAGES][2];  // constant gains per stage and channel (used when the ramp bit is clear)
};
static_assert(sizeof(VoiceBlk) == 96, "VoiceBlk layout");

// Compact per (block, voice) record (16 B): all the leaf kernel needs for silent and VB_SIMPLE blocks.  Only
// blocks that are neither (ramps, loop wrap, one-shot tail, non-planar-f32 sources) also get a full VoiceBlk.
// VB_SIMPLE source classes (bits 16..18 of VoiceRef::flags_gset): how the leaf kernel fetches 4 consecutive frames
enum : uint32_t {
    SF_P_F32 = 0,  // planar f32 (also interleaved mono): dwordx4 per channel
    SF_P_I16 = 1,  // planar i16 (also interleaved mono), 4-byte aligned: dwordx2 per channel
    SF_P_U16 = 2,
    SF_I_I16 = 3,  // interleaved stereo i16: ONE dwordx4 holds both channels of 4 frames
    SF_I_U16 = 4,
    SF_I_F32 = 5,  // interleaved stereo f32: two dwordx4
    SF_NONE = 7,   // not eligible for the compact fast path
};
struct VoiceRef {
    const float* src_l;  // VB_SIMPLE: address of channel 0 of the block's first frame (typed by the source class)
    uint32_t r_delta;    // VB_SIMPLE: channel-1 offset in source ELEMENTS (0 for a mono sample)
    uint32_t flags_gset; // bits 0..7 VB_* flags, bits 8..15 gain-set index, bits 16..18 source class (SF_*)
};
static_assert(sizeof(VoiceRef) == 16, "VoiceRef layout");
#define FW_GSETS 4  // distinct constant-gain sets a voice may use inside one call before falling back to VoiceBlk
struct GainSet {
    float g[FW_MAX_STAGES][2];
};

// Per voice, across calls: "this voice ended the last call steady" + the descriptor its blocks share.
// Valid only while epoch == FusedView::epoch (the host bumps it on every plan install / sample-table change).
struct VoiceCache {
    uint32_t epoch;
    int mode;
    uint32_t flags;
    int sample;
    GainSet g;
};
static_assert(sizeof(VoiceCache) == 64, "VoiceCache layout");

// (host side, here so that the test harness can reach it) quiet_window's look-ahead rule, no call being in flight at `now` (all steady_clock ns): the last call began at `start`, `period`
// after the one before, and took `dur`.  true: the next call is due within `margin` — wait for it to come and go.  false: go now
// (room before the next call; or no rhythm known; or a stream without gaps of 2 x margin to use; or the call is overdue by more
// than the margin: a stream that stopped must not hold a build up).
inline bool quiet_next_call_is_due(uint64_t now, uint64_t start, uint64_t period, uint64_t dur, uint64_t margin) {
    if (!period || period > 200000000ull || period < dur + 2 * margin) return false;
    const uint64_t since = now - start;
    return !(since + margin < period || since > period + margin);
}
// plan build: one piece of the build's device work (k_build_apply).  src != nullptr: copy row_bytes from pinned host memory
// (rows = 1); src == nullptr: rows x row_bytes at `pitch` bytes set to `value`, byte 0 of every row to `head` if head >= 0
struct BuildJob {
    void* dst;
    const void* src;
    unsigned long long row_bytes, pitch;
    uint32_t rows, value;
    int head, pad_;
};
static_assert(sizeof(BuildJob) == 48, "BuildJob layout");

// plan adoption: which steady caches travel from the old plan to the new one (k_adopt_init / carry_cache_voice); n_new = 0: none
// Round 4 — "lazy" records.  A voice that ends a call STEADY (constant gains, nothing but the playhead moving) and whose blocks
// are all plain ones (silent, or a contiguous planar-f32 source that never wraps inside a block) has records that are a pure
// function of (this record, block index): the control kernel writes one of these per voice at the end of a call, and the NEXT
// calls — as long as they carry no message, the plan has not changed and the host has SEEN that every voice of the plan left
// one behind (FusedView::horizon -> pinned memory) — are rendered without a control kernel at all: the leaf wave's lane p loads
// port p's LazyRec (descriptor AND gains: one round trip where records + gain sets were two) and computes the block's source
// address itself.  Node state is brought up to date (k_lazy_flush) before anything else reads it.
struct LazyRec {
    uint64_t base;        // BYTE address of source frame 0 of the record: mode 1: the loop start; mode 2: the sample's start; mode 0: unused
    uint64_t off0;        // mode 2: playhead (frames) at the record's block 0
    uint64_t loop_start;  // mode 1 (k_lazy_flush rebuilds the playhead from it)
    uint32_t r_delta;     // the record's r_delta (channel-1 offset in elements; 0 = mono)
    uint32_t flags_gset;  // the record's flags_gset (gain-set index bits unused: the gains are `g` below)
    uint32_t q;           // mode 1: loop length in BLOCKS
    uint32_t r0b;         // mode 1: playhead offset from the loop start at the record's block 0, in blocks
    uint32_t frames;      // block size the block counts refer to
    int mode;             // 0 nothing moves, 1 looping playhead, 2 one-shot playhead (TailJob::mode); -1 = not lazy-capable
    int sampler_state;    // the voice's sampler state slot (-1: a null voice)
    uint32_t bpf;         // bytes per source frame at `base` (the record's source class: planar f32 4, planar 16-bit 2, interleaved
                          // stereo 16-bit 4, interleaved stereo f32 8)
    uint32_t pad[2];
    GainSet g;
    uint32_t pad2[4];
};
static_assert(sizeof(LazyRec) == 128, "LazyRec layout");

struct VoiceDesc;
struct CarryArgs {
    VoiceCache* new_cache;
    const VoiceDesc* new_voices;
    int n_new;
    const VoiceCache* old_cache;
    const VoiceDesc* old_voices;
    const int* old_slot_voice;
    int n_old_slots;
    uint32_t old_epoch, new_epoch;
};

// ---------------------------------------------------------------- FIR convolution bank (MFMA GEMM)
#define FIR_SEG 4096  // window positions per split-K segment — part of the numeric SPEC (summation order)
#ifndef FIR_KC
#define FIR_KC 128    // window positions staged per LDS chunk (64 or 128; not part of the numeric SPEC)
#endif
struct FirRow {  // one GEMM row = one channel of one FIR node
    int state;
    int ch;
    int in_buf;
    int out_buf;
};
// K_FIR, morph-capable (SPEC FIR morph): a FIR node created with two or more parameters has two impulse-response slots
// A and B of T taps each (a shorter impulse response is zero-padded to T) over ONE history ring per channel.  The slot sums s_A[n],
// s_B[n] are the plain FIR definition above (segments of FIR_SEG, fma chains from +0.0, partials added in order, + (+0.0f)); an empty
// slot's sum is +0.0.  The position p of frame n follows the crossfader's rule (XfSeg, xf_positions: node time = frames rendered since
// activation, a message retargets from where the old segment stands), the gains its laws (xf_gains), and
//     y[n] = s_A[n] if p == 0,  s_B[n] if p == 1,  else (s_A[n] * a) + (s_B[n] * b)      (three separately rounded operations)
// A block is at rest when dur == 0 or the segment has ended at its first frame; at rest at p == 0 slot B is idle for the block (no
// matrix work), at rest at p == 1 slot A is, in every other block both slots run.
// State, in NodeState fields a plain FIR node leaves at make_state's values (playhead, loop_start, loop_end, sample, ext_off, ext_len
// mean what they mean for every FIR node; the ext slice is the rings, then — 16-float aligned — one FirMorphBlk per block of a batch):
//     enabled = 1 (0: a plain node), s0.status = 0 (1: a creation parameter was refused), p0 / p1 = P0 / P1, full_range = dur,
//     has_loop = shape, phasor, phasor_inc, gain, aux = x1, y1, x2, y2, playing = law, s0.input | s0.last << 32 = node time (raw bits),
//     s0.a | s0.b << 32 = t0, s1.input = ext offset of the block records, s1.last = how many there are (raw bits);
//     s1.status / s1.a carry the creation parameters ir_b / max_taps to the host's bookkeeping (no kernel reads them)
// Rows (FirRow) of a morph group: an A row is a plain row; a B row names the same state and ch, in_buf = -1 (that is what marks it)
// and its node's out_buf.  Behind the group's n_rows / 32 tile offsets sit n_rows partner indices: row r's other slot's row in the
// group, FIR_NO_PARTNER for none.
#define FIR_MORPH_BLK_FLOATS 16
#define FIR_NO_PARTNER 0xffffffffu
#define FIR_MORPH_GROUP 0x80000000u  // DevView::fir_morph: the flag; the bits below it are the batch's first block
enum : int { FIR_MODE_NONE = 0, FIR_MODE_A = 1, FIR_MODE_B = 2, FIR_MODE_BOTH = 3 };  // bit 0: slot A runs, bit 1: slot B runs
struct FirMorphBlk {  // what k_fir_morph_control leaves per block of the batch: the segment in force at the block's first frame
    float P0, P1, x1, y1, x2, y2;
    uint32_t t0_lo, t0_hi, dur;
    int shape;
    uint32_t T_lo, T_hi;  // node time of the block's first frame
    int mode, law;
    uint32_t pad[2];
};
static_assert(sizeof(FirMorphBlk) == FIR_MORPH_BLK_FLOATS * sizeof(float), "FirMorphBlk layout");
FW_TYPES_HD inline bool fir_morph_on(const NodeState& s) { return s.enabled == 1; }
FW_TYPES_HD inline uint64_t fir_morph_time(const NodeState& s) { return (uint64_t)fw_bits_of(s.s0.input) | ((uint64_t)fw_bits_of(s.s0.last) << 32); }
FW_TYPES_HD inline void fir_morph_set_time(NodeState& s, uint64_t t) {
    s.s0.input = fw_float_of((uint32_t)t);
    s.s0.last = fw_float_of((uint32_t)(t >> 32));
}
FW_TYPES_HD inline uint64_t fir_morph_t0(const NodeState& s) { return (uint64_t)fw_bits_of(s.s0.a) | ((uint64_t)fw_bits_of(s.s0.b) << 32); }
FW_TYPES_HD inline uint32_t fir_morph_tab(const NodeState& s) { return fw_bits_of(s.s1.input); }
FW_TYPES_HD inline uint32_t fir_morph_tab_n(const NodeState& s) { return fw_bits_of(s.s1.last); }
FW_TYPES_HD inline XfSeg fir_morph_seg(const NodeState& s) {
    return XfSeg{s.p0, s.p1, s.phasor, s.phasor_inc, s.gain, s.aux, fir_morph_t0(s), (uint32_t)s.full_range, s.has_loop};
}
FW_TYPES_HD inline XfSeg fir_morph_seg(const FirMorphBlk& b) {
    return XfSeg{b.P0, b.P1, b.x1, b.y1, b.x2, b.y2, (uint64_t)b.t0_lo | ((uint64_t)b.t0_hi << 32), b.dur, b.shape};
}
// where the rings end and the block records begin, and the whole slice, in floats (nch rings of 2R, `n_blk` records)
FW_TYPES_HD inline uint32_t fir_morph_tab_rel(uint64_t R, uint32_t nch) { return (uint32_t)(((uint64_t)nch * 2u * R + 15u) / 16u * 16u); }
FW_TYPES_HD inline uint64_t fir_morph_ext_len(uint64_t R, uint32_t nch, uint32_t n_blk) {
    return (uint64_t)fir_morph_tab_rel(R, nch) + (uint64_t)n_blk * FIR_MORPH_BLK_FLOATS;
}
// the states the morph kernels render (anything else would index the ext pool out of bounds): ONE statement for the plan build, the
// device guard of k_fir_morph_control and a host build
FW_TYPES_HD inline bool fir_morph_state_ok(const NodeState& s, int n_in, int n_out) {
    const auto unit = [](float x) { return x >= 0.0f && x <= 1.0f; };  // (false for a NaN)
    const auto ctl_y = [](float y) { return y >= -1.0f && y <= 2.0f; };
    const int nch = n_in < n_out ? n_in : n_out;
    const uint64_t T = s.loop_start, R = s.loop_end;
    if (!(s.enabled == 1 && s.s0.status == 0 && nch >= 1 && T >= 1 && T <= (1u << 24) && R >= T && s.playhead < R)) return false;
    if (!(unit(s.p0) && unit(s.p1) && s.full_range >= 0 && (uint32_t)s.full_range <= XF_FRAMES_MAX &&
          (s.has_loop == XF_SHAPE_LINEAR || s.has_loop == XF_SHAPE_BEZIER) && (s.playing == XF_LAW_LINEAR || s.playing == XF_LAW_EQUAL_POWER) &&
          unit(s.phasor) && unit(s.gain) && ctl_y(s.phasor_inc) && ctl_y(s.aux) && fir_morph_time(s) >= fir_morph_t0(s)))
        return false;
    const uint64_t tab = fir_morph_tab(s), n_blk = fir_morph_tab_n(s);
    return n_blk >= 1 && tab % 16u == 0 && tab >= (uint64_t)s.ext_off + (uint64_t)nch * 2u * R &&
           tab + n_blk * FIR_MORPH_BLK_FLOATS <= (uint64_t)s.ext_off + (uint64_t)s.ext_len;
}
// CMD_XF_TO at a block's first frame: a new segment from where the old one stands (the crossfader's retarget rule)
FW_TYPES_HD inline void fir_morph_msg(NodeState& s, float P1, uint32_t frames, int shape, float x1, float y1, float x2, float y2) {
    float from[1];
    const uint64_t T = fir_morph_time(s);
    xf_positions<1>(fir_morph_seg(s), T, from);
    s.p0 = from[0];
    s.p1 = P1;
    s.s0.a = fw_float_of((uint32_t)T);
    s.s0.b = fw_float_of((uint32_t)(T >> 32));
    s.full_range = (int)frames;
    s.has_loop = shape;
    s.phasor = x1;
    s.phasor_inc = y1;
    s.gain = x2;
    s.aux = y2;
}
FW_TYPES_HD inline int fir_morph_mode(const XfSeg& g, uint64_t T) {
    const bool rest = g.dur == 0u || T - g.t0 >= (uint64_t)g.dur;
    return rest && g.P1 == 0.0f ? FIR_MODE_A : (rest && g.P1 == 1.0f ? FIR_MODE_B : FIR_MODE_BOTH);
}
// one block of `frames` frames, its messages applied: the record, then the advanced time
FW_TYPES_HD inline FirMorphBlk fir_morph_block(NodeState& s, uint32_t frames) {
    const XfSeg g = fir_morph_seg(s);
    const uint64_t T = fir_morph_time(s);
    FirMorphBlk b = {g.P0, g.P1, g.x1, g.y1, g.x2, g.y2, (uint32_t)g.t0, (uint32_t)(g.t0 >> 32), g.dur, g.shape, (uint32_t)T, (uint32_t)(T >> 32),
                     fir_morph_mode(g, T), s.playing, {0u, 0u}};
    fir_morph_set_time(s, T + (uint64_t)frames);
    return b;
}
// frame n (node time) of a block whose record is b, from the two slot sums (an idle or empty slot's: +0.0f, never read at its end)
FW_TYPES_HD_INLINE float fir_morph_out(const FirMorphBlk& b, const XfSeg& g, uint64_t n, float sA, float sB) {
    if (b.mode == FIR_MODE_A) return sA;
    if (b.mode == FIR_MODE_B) return sB;
    float p[1], ga, gb;
    xf_positions<1>(g, n, p);
    if (p[0] == 0.0f) return sA;
    if (p[0] == 1.0f) return sB;
    xf_gains(b.law, p[0], ga, gb);
    return (sA * ga) + (sB * gb);
}

#define CH_FAST_KMAX 64  // blocks per k_chain launch its steady-call loop keeps per-block source addresses for (LDS);
                         // the host never batches more blocks than this into one chain-plan launch

// grouped calls (k_leaf.hip.h k_leaf_group_lazy): the default of the FWGPU_LEAF_GROUP switch, and the smallest K x pieces that is grouped
#ifndef FWGPU_LEAF_GROUP_DEFAULT
#define FWGPU_LEAF_GROUP_DEFAULT true
#endif
#ifndef FWGPU_LEAF_GROUP_MIN_DEFAULT
// measured (profiles/leaf_group_sizes.jsonl; ms per call grouped / two kernels): 16 items 0.133 / 0.019, 64 items 0.135 / 0.032, 256 items
// (block 1024 x K = 64) 0.150 / 0.102, 768 items 0.260 / 0.288 — a workgroup walks all the root's leaves, ~130 us whatever the grid, so the
// call pays only once the grid gives every CU work: 768 is the smallest measured size at which the grouped call is not slower
#define FWGPU_LEAF_GROUP_MIN_DEFAULT 768u
#endif
// the root SumNode of a fused plan, passed to k_root_out by value (kernel arguments: scalar loads, no dependent fetch)
struct RootArgs {
    int n_in, ports;  // ports = n_in / 2 stereo ports (<= 32)
    int in_buf[64];   // bus buffer of input channel i
    const int* in_tab;  // the same table in device memory (for per-lane indexing)
    int grouped;        // 1: k_leaf_group_lazy rendered this batch's root already (a grouped call, fwgpu_run.cpp): launch_root_out launches
                        // nothing.  0 in the plan's own copy and on every other path.
    int pad_;
};

// k_chain plan: what the two channel workgroups of a voice share, as it stood at the START of the current call
// (written by k_voice_control, which also advances the node state to the end of the call; read-only for k_chain)
struct ChainStart {
    uint32_t pos;       // delay ring position
    float fb, mix, dry; // delay feedback / wet / dry
    float co[5];        // biquad b0 b1 b2 a1 a2
    float co2[5];       // the second biquad's (VoiceDesc::bq2_state)
    uint32_t pad[2];    // per biquad: 1 = a sweep was in flight at the call's start — its state is the snapshot behind the node's ext slice
};
static_assert(sizeof(ChainStart) == 64, "ChainStart layout");

// the top-level SumNode over the partial mix buses of R voice shards (nodes/sum.rs:111-133), passed by value
#define FW_MAX_BUS_PARTS 64
struct BusParts {
    int n;
    const float* part[FW_MAX_BUS_PARTS];  // part[r] = rank r's interleaved bus (peer-mapped or all-gathered), same length each
};

// one-shot mix-bus exchange over peer-mapped slots (k_exchange.hip.h): what every rank of an exchange agrees on ...
struct ExchangeGeom {
    int world, rank;
    uint64_t max_floats;  // floats of one slot's bus
    uint64_t slot_bytes;  // max_floats * 4 + silence bytes, padded to 256
};
// ... and where each rank's region is mapped in THIS process (base[rank] = its own), passed by value
struct ExchangePeers {
    char* base[FW_MAX_BUS_PARTS];
};

#define CH_GROUP_LEAVES 8
// k_chain workgroup = up to CH_GROUP_LEAVES consecutive leaf SumNodes with at most 32 voices together (their voices are
// consecutive): a tree of small leaves (a bus per instrument) fills the workgroup's 32 voice rows like one wide leaf
struct ChainGroup {
    int first_voice, n_voices;
    int n_leaves;
    int uniform_ports;     // 32 / 16 / 8 / 4: the 32 rows are full leaves of exactly that many ports; 0 otherwise
    uint32_t start_mask;   // bit r: voice row r is port 0 of a leaf
    uint32_t masked_rows;  // bit r: row r belongs to a leaf on the n-port path (ports not 2, 3 or 4): silent ports skipped
    int out_buf[CH_GROUP_LEAVES];  // per leaf: compact bus-buffer id of output channel 0
    int row0[CH_GROUP_LEAVES];     // per leaf: its first voice row
    int ports[CH_GROUP_LEAVES];
};

struct LeafDesc {  // a SumNode whose ports are all voice chains (nodes/sum.rs)
    int first_voice;
    int ports;     // num_in_ports
    int out_buf;   // compact bus-buffer id of output channel 0 (channel 1 = +1)
    int pad;       // when set: the port count of the WHOLE SumNode (this leaf is its leading voice ports): decides the
                   // masked / unmasked path (Q13) instead of `ports`
};

}  // namespace fwgpu
