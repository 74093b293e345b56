// k_compressor.hip.h — SPEC bus compressor (K_COMPRESSOR): a kernel of its own next to k_level, as k_limiter and k_ducker
// are, so that its LDS (the staged gain targets) is paid by no other node kind.  Included by fwgpu_kernels.hip.
//
// n channels in, n out, self-keyed, linked.  Per frame n since activation (q[n < 0] = 65535; a channel flagged silent for a block counts
// as +0.0 and is not read):
//   key[n] = max_c |x_c[n]| (fmaxf from +0.0)       u[n] = key[n] / T0
//   t[n]   = 1.0f if !(u > 1.0f), else with d = bits(u) - 0x3F800000, i = d >> 19, fr = (float)(d & 0x7FFFF) * 2^-19:
//            G[320] if i >= 320, else G[i] + ((G[i+1] - G[i]) * fr)                                         (no FMA)
//   q[n]   = (uint32)((t[n] * 65535.0f) + 0.5f)      m[n] = min of q[k], k in [n-H, n]
//   ca[n]  = sum of m[k], k in (n-A, n]              cr[n] = sum of m[k], k in (n-R, n]                      (integers below 2^31)
//   g[n]   = fminf((float)ca / (float)(A * 65535), (float)cr / (float)(R * 65535))         y_c[n] = x_c[n] * (g[n] * M)
// No recurrence in time: a frame is a function of the W = max(A, R) + H values of q in front of it and its own.  One workgroup takes a
// node and a RUN of consecutive blocks of the batch (or, where a block is longer than COMP_RUN_MAX frames, a piece of one block):
//   (1) q of the W frames in front of the run and of the run itself into LDS, 16 bits each: in front of the batch's first frame from
//       the node's stored history (which holds 65535 - q), from there on from the input buffers of this and the earlier blocks of the
//       batch, which the level above has written for the whole batch; a thread a frame, four frames' loads in flight together;
//   (2) the hold: a sliding minimum over H + 1 frames by doubling in place — m = min(m, m shifted by 2^j), then one overlapping
//       minimum — every group of values read before it is written;
//   (3) ca and cr at the frame in front of the run: a workgroup reduction over the staged values;
//   (4) inside the run c[n] = c[n-1] + m[n] - m[n-L]: four consecutive frames per thread, a wave prefix scan over the threads' sums
//       and the waves' totals through LDS; then a, r, g and the channels times g * M, 16 bytes per thread and channel, non-temporal.
// LDS: consecutive threads read consecutive 16-bit values, so two lanes share a dword and a wave's read covers 32 banks once — the
// pairs are broadcasts, no conflict; the four values of a thread in (4) start at any parity, so they are four 16-bit reads.
// The history the batch leaves behind — the last W values of (history ++ the batch's q) — is written where no workgroup of the launch
// still reads the old one: by k_compressor_hist, launched right behind k_compressor (stream order is the barrier), or, where one
// workgroup renders the whole launch (one block in one piece; fwgpu_node_process), by that workgroup when it is done.
#define COMP_THREADS 256
#define COMP_STR_MAX (COMP_WIN_MAX + COMP_HOLD_MAX + COMP_RUN_MAX)  // 38 912 staged values
struct CompLds {
    float G[COMP_TAB_PAD];
    int tot[2][2][COMP_THREADS / WAVE];  // [chunk parity][A-window, R-window][wave]: the waves' totals of a chunk
    uint32_t red[2][COMP_THREADS / WAVE];
    uint16_t q[COMP_STR_MAX + 8];        // 77 840 bytes; the whole struct 79 248: two workgroups to a CU's 163 840
};

// what one workgroup knows about its node
struct CompP {
    float T0, M, Af, Rf;
    int A, R, H, W;
    int n;
    const float* tab;   // G[COMP_TAB_PAD]
    uint32_t* hist;     // (W + 1) / 2 slots of two 16-bit words: 65535 - q, oldest first
    const int* in_buf;
    const int* out_buf;
};
// false: state a plan build would not let through (a slice of another size would be indexed out of bounds)
__device__ __forceinline__ bool comp_params(const DevView& v, const NodeDesc& nd, const NodeState& s, CompP& p) {
    if (!comp_state_ok(s, nd.n_in, nd.n_out) || s.ext_len != comp_ext_len(s) || v.frames < 1 || v.frames > v.stride) return false;
    p.T0 = s.p0;
    p.M = s.p1;
    p.A = (int)s.playhead;
    p.R = (int)s.loop_start;
    p.H = s.full_range;
    p.W = (int)s.loop_end;
    p.Af = (float)((uint32_t)p.A * 65535u);
    p.Rf = (float)((uint32_t)p.R * 65535u);
    p.n = nd.n_out;
    p.tab = v.ext + s.ext_off;
    p.hist = (uint32_t*)(v.ext + s.ext_off + COMP_TAB_PAD);
    p.in_buf = v.in_buf + nd.in_off;
    p.out_buf = v.out_buf + nd.out_off;
    return true;
}
// q[] at frame g of the batch (0 <= g < K * frames); G: the table, in LDS or in the ext slice
__device__ __forceinline__ uint32_t comp_q(const DevView& v, const CompP& p, const float* G, uint32_t g) {
    const uint32_t blk = g / (uint32_t)v.frames, f = g - blk * (uint32_t)v.frames;
    const float* pool = v.pool + (size_t)blk * v.pool_blk_stride;
    const uint8_t* fl = v.flags + (size_t)blk * v.flags_blk_stride;
    float key = 0.f;
    for (int c = 0; c < p.n; ++c) {
        const int buf = p.in_buf[c];
        if (!fl[buf]) key = fmaxf(key, fabsf(pool[(size_t)buf * v.stride + f]));  // (a NaN sample is ignored)
    }
    const float u = key / p.T0;
    float t = 1.0f;
    if (u > 1.0f) {
        const uint32_t d = fw_bits_of(u) - 0x3F800000u, i = d >> 19;
        if (i >= (uint32_t)(COMP_TAB_N - 1)) {
            t = G[COMP_TAB_N - 1];
        } else {
            const float fr = (float)(d & 0x7FFFFu) * 0x1p-19f;
            const float g0 = G[i];
            t = g0 + ((G[i + 1] - g0) * fr);
        }
    }
    return (uint32_t)((t * 65535.0f) + 0.5f);
}
// value h of the stored history (0 <= h < W) as q
__device__ __forceinline__ uint32_t comp_hist_q(const CompP& p, int h) { return 65535u - ((p.hist[h >> 1] >> ((h & 1) * 16)) & 0xFFFFu); }

// m[i] = min(m[i], m[i - sft]) over the S staged values, in place: a value reads values below it, so the groups go from the top down
__device__ __forceinline__ void comp_shift_min(CompLds& L, int S, int sft) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int r0 = ((S - 1) / (8 * nt)) * (8 * nt); r0 >= 0; r0 -= 8 * nt) {
        uint16_t a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = r0 + e * nt + tid;
            a[e] = 0xFFFFu;
            if (i < S) {
                a[e] = L.q[i];
                if (i >= sft) {
                    const uint16_t b = L.q[i - sft];
                    a[e] = b < a[e] ? b : a[e];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = r0 + e * nt + tid;
            if (i < S) L.q[i] = a[e];
        }
    }
    __syncthreads();
}
// the sum of the staged values [lo, hi), 0 <= lo < hi, at most 32768 of them: the same number in every thread (slot: which of the two
// reduction rows — two sums in a row need no barrier between them)
__device__ __forceinline__ uint32_t comp_sum(CompLds& L, int lo, int hi, int slot) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (WAVE - 1), nw = nt / WAVE;
    uint32_t s = 0u;
    for (int i = lo + tid; i < hi; i += nt) s += L.q[i];
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) s += __shfl_xor(s, h);
    if (lane == 0) L.red[slot][tid / WAVE] = s;
    __syncthreads();
    uint32_t r = 0u;
    for (int w = 0; w < nw; ++w) r += L.red[slot][w];
    return r;
}

// run `run` of the launch's K blocks; every thread of the workgroup comes here (blockDim.x: a multiple of WAVE, at most COMP_THREADS)
__device__ void compressor_run(const DevView& v, const CompP& p, uint32_t run, uint32_t K, CompLds& L) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (WAVE - 1), wave = tid / WAVE, nw = nt / WAVE;
    const int frames = v.frames;
    // which frames: whole blocks, about a window's worth of them so that the staged window is shared (a workgroup per block would stage
    // W frames for every block), or one piece of a block longer than COMP_RUN_MAX
    uint32_t b0, nb;
    int f_lo = 0, f_hi = frames;
    if (frames <= COMP_RUN_MAX) {
        const int target = p.W < 1024 ? 1024 : (p.W > COMP_RUN_MAX ? COMP_RUN_MAX : p.W);
        const uint32_t bpr = target / frames > 1 ? (uint32_t)(target / frames) : 1u;
        b0 = run * bpr;
        if (b0 >= K) return;
        nb = K - b0 < bpr ? K - b0 : bpr;
    } else {
        const uint32_t ppb = (uint32_t)((frames + COMP_RUN_MAX - 1) / COMP_RUN_MAX);
        b0 = run / ppb;
        if (b0 >= K) return;
        nb = 1;
        f_lo = (int)(run % ppb) * COMP_RUN_MAX;
        f_hi = frames - f_lo < COMP_RUN_MAX ? frames : f_lo + COMP_RUN_MAX;
    }
    const int Ln = nb == 1 ? f_hi - f_lo : (int)nb * frames;  // <= COMP_RUN_MAX
    const int gs = (int)b0 * frames + f_lo;                    // the run's first frame, counted from the batch's
    const int W = p.W, S = W + Ln;                             // staged value i is frame gs - W + i; S <= COMP_STR_MAX
    __syncthreads();  // (fwgpu_node_process takes the pieces of a long block one after the other)
    for (int i = tid; i < COMP_TAB_PAD; i += nt) L.G[i] = p.tab[i];
    __syncthreads();
    // (1) the gain targets
    for (int i0 = 0; i0 < S; i0 += 4 * nt) {
        uint32_t qv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + e * nt + tid, g = gs - W + i;
            qv[e] = 65535u;
            if (i < S) qv[e] = g < 0 ? comp_hist_q(p, W + g) : comp_q(v, p, L.G, (uint32_t)g);  // (g >= -W)
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + e * nt + tid;
            if (i < S) L.q[i] = (uint16_t)qv[e];
        }
    }
    __syncthreads();
    // (2) the hold: m = the minimum over H + 1 values.  2^P <= H + 1 < 2^(P+1): P doublings leave the minimum over 2^P, two of those
    // overlapping the minimum over H + 1.  Values [0, H) see less than their window; none of them is in a window sum (W - max(A, R) = H)
    if (p.H > 0) {
        const int Lw = p.H + 1, P = 31 - __builtin_clz(Lw);
        for (int j = 0; j < P; ++j) comp_shift_min(L, S, 1 << j);
        if (Lw > (1 << P)) comp_shift_min(L, S, Lw - (1 << P));
    }
    // (3) the sums at the frame in front of the run (A, R <= W: the windows are staged)
    int ca = (int)comp_sum(L, W - p.A, W, 0), cr = (int)comp_sum(L, W - p.R, W, 1);
    // (4) block by block, 4 * blockDim.x frames at a time, four consecutive frames per thread
    int pos = W, par = 0;
    for (uint32_t ib = 0; ib < nb; ++ib) {
        const uint32_t blk = b0 + ib;
        float* pool = v.pool + (size_t)blk * v.pool_blk_stride;
        uint8_t* fl = v.flags + (size_t)blk * v.flags_blk_stride;
        uint32_t silent = 0u;
        for (int c = 0; c < p.n; ++c) silent |= fl[p.in_buf[c]] != 0 ? 1u << c : 0u;
        for (int cf = f_lo; cf < f_hi; cf += 4 * nt) {
            const int f0 = cf + 4 * tid;
            const int valid = f_hi - f0 >= 4 ? 4 : (f_hi - f0 > 0 ? f_hi - f0 : 0);
            const int x = pos + (f0 - f_lo);
            int pa[4], pr[4];  // the thread's own inclusive sums of (entering - leaving)
            int sa = 0, sr = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e < valid) {  // (x + e < S; x + e - A, x + e - R >= W - max(A, R) >= 0)
                    const int en = (int)L.q[x + e];
                    sa += en - (int)L.q[x + e - p.A];
                    sr += en - (int)L.q[x + e - p.R];
                }
                pa[e] = sa;
                pr[e] = sr;
            }
            // inclusive scan over the wave, then the waves in front through LDS (|sums| <= 4 * blockDim.x * 65535 < 2^27)
            int ia = sa, ir = sr;
#pragma unroll
            for (int h = 1; h < WAVE; h <<= 1) {
                const int ta = __shfl_up(ia, h), tr = __shfl_up(ir, h);
                if (lane >= h) {
                    ia += ta;
                    ir += tr;
                }
            }
            if (lane == WAVE - 1) {
                L.tot[par][0][wave] = ia;
                L.tot[par][1][wave] = ir;
            }
            __syncthreads();  // (one per chunk: the totals alternate between two rows)
            int ba = ca + ia - sa, br = cr + ir - sr;  // the sums at the frame in front of this thread's four
            for (int w = 0; w < nw; ++w) {
                const int ta = L.tot[par][0][w], tr = L.tot[par][1][w];
                if (w < wave) {
                    ba += ta;
                    br += tr;
                }
                ca += ta;
                cr += tr;
            }
            par ^= 1;
            v4f g;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = (float)(uint32_t)(ba + pa[e]) / p.Af;
                const float r = (float)(uint32_t)(br + pr[e]) / p.Rf;
                g[e] = fminf(a, r) * p.M;
            }
            if (valid)
                for (int c = 0; c < p.n; ++c) {
                    float* out = pool + (size_t)p.out_buf[c] * v.stride + f0;
                    v4f y = splat(0.f);  // (a channel flagged silent is not read: zeros out, flagged)
                    if (!((silent >> c) & 1u)) {
                        const v4f xin = __builtin_nontemporal_load((const v4f*)(pool + (size_t)p.in_buf[c] * v.stride + f0));
                        y = xin * g;
                    }
                    __builtin_nontemporal_store(y, (v4f*)out);
                }
        }
        pos += f_hi - f_lo;
        // the meter's pass-through rule; nothing else is ever flagged
        if (tid < p.n) fl[p.out_buf[tid]] = (silent >> tid) & 1u ? 1 : 0;
    }
}

// the history a launch of K blocks leaves behind: new[i] = S[i + K * frames], S = old history ++ the batch's q.  A shift of the slice in
// place where the batch is shorter than W: groups of blockDim.x slots go up, every load of a group is back before its first store, and
// no group reads what an earlier one wrote.  Every thread of the workgroup comes here.
__device__ void compressor_history(const DevView& v, const CompP& p, uint32_t K) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const long long total = (long long)K * v.frames;
    const int nslots = (p.W + 1) >> 1;
    __syncthreads();
    for (int t0 = 0; t0 < nslots; t0 += nt) {
        const int t = t0 + tid;
        uint32_t word = 0u;
        if (t < nslots) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i = 2 * t + e;  // value of the new history
                const long long x = (long long)i + total;
                uint32_t q = 65535u;      // (the value behind the last one of an odd W stays 0)
                if (i < p.W) q = x < p.W ? comp_hist_q(p, (int)x) : comp_q(v, p, p.tab, (uint32_t)(x - p.W));
                word |= (65535u - q) << (16 * e);
            }
        }
        __syncthreads();
        if (t < nslots) p.hist[t] = word;
    }
    __syncthreads();
}

// one workgroup per (node of the level, run); nodes of other kinds are k_level's.  own_hist: the launch is one run, and its workgroup
// writes the history back itself
__global__ __launch_bounds__(COMP_THREADS) void k_compressor(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K, int own_hist) {
    __shared__ CompLds L;
    if ((int)blockIdx.x >= n_nodes) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_COMPRESSOR) return;
    CompP p;
    if (!comp_params(v, nd, v.states[nd.state], p)) return;
    compressor_run(v, p, blockIdx.y, K, L);
    if (own_hist && blockIdx.y == 0) compressor_history(v, p, K);
}
// the follow-up of a launch of more than one run: one workgroup per node
__global__ __launch_bounds__(COMP_THREADS) void k_compressor_hist(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K) {
    if ((int)blockIdx.x >= n_nodes) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_COMPRESSOR) return;
    CompP p;
    if (!comp_params(v, nd, v.states[nd.state], p)) return;
    compressor_history(v, p, K);
}
