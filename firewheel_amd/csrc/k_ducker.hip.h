// k_ducker.hip.h — SPEC sidechain ducker (K_DUCKER): a kernel of its own next to k_level, as k_limiter is, so that its LDS
// (the staged gate bits) and its registers are paid by no other node kind.  Included by fwgpu_kernels.hip.
//
// Inputs 0..n-1 are the main bus x_c, inputs n..n+k-1 the key k_j (never heard).  Per frame n since activation (everything false / zero
// for n < 0, a key channel flagged silent counts as +0.0 and is not read):
//   key[n]  = max_j |k_j[n]| (fmaxf from +0.0)      on[n]   = key[n] > T
//   open[n] = on[k] for some k in [n-H, n]           ca[n]   = #open in (n-A, n]        cr[n] = #open in (n-R, n]       (integers)
//   u[n]    = fmaxf((float)ca / (float)A, (float)cr / (float)R)                          g[n]  = 1.0f - ((1.0f - D) * u[n])   (no FMA)
//   y_c[n]  = x_c[n] * g[n]
// No recurrence in time: a frame is a function of the W = max(A, R) + H gate bits in front of it and its own.  One wave takes a node and
// a RUN of consecutive blocks of the batch (or, where a block is longer than DUCK_RUN_MAX frames, a piece of one block):
//   (1) the `on` bits of the W frames in front of the run and of the run itself into LDS, 64 frames per word: a __ballot over the key
//       buffers of this and the earlier blocks of the batch (the level above has written them for the whole batch), and in front of the
//       batch's first frame the node's stored history, aligned by a funnel shift;
//   (2) the hold: a dilation of the bit string by H, by doubling in place on the words — w |= w << 2^j, then one overlapping OR —
//       every group of words read before it is written;
//   (3) ca and cr at the frame in front of the run: popcounts over the words, an integer wave reduction; inside the run
//       c[n] = c[n-1] + open[n] - open[n-L], a wave prefix scan over the lanes' popcounts of four frames each;
//   (4) a, r, u, g per frame, and the main channels times g: 16 bytes per lane and channel, non-temporal.
// The history the batch leaves behind — the last W bits of (history ++ the batch's bits) — is written where no wave of the launch still
// reads the old one: by k_ducker_hist, a wave per node launched right behind k_ducker (stream order is the barrier), or, where one wave
// renders the whole launch (one block in one piece; fwgpu_node_process), by that wave when it is done.
#define DUCK_LDS_WORDS ((DUCK_WIN_MAX + DUCK_HOLD_MAX + DUCK_RUN_MAX) / 64 + 2)  // 1154 words of 64 bits: 9232 bytes
struct DuckLds {
    unsigned long long b[DUCK_LDS_WORDS];
};

// what one wave knows about its node
struct DuckP {
    float T, dd, Af, Rf;
    int A, R, H, W;
    int n, k;          // main channels, key channels
    int nw32;          // 32-bit words of the stored history: 2 * ceil(W / 64)
    uint32_t* hist;    // ... oldest first, bit i in bit i % 32 of word i / 32; the bits from W on are zero
    const int* in_buf;
    const int* out_buf;
};
// false: state a plan build would not let through — the host harness holds it to that (a slice of another size would be indexed out
// of bounds)
__device__ __forceinline__ bool duck_params(const DevView& v, const NodeDesc& nd, const NodeState& s, DuckP& p) {
    if (!duck_state_ok(s, nd.n_in, nd.n_out) || s.ext_len != duck_ext_len(s) || v.frames < 1) return false;
    p.T = s.p0;
    p.dd = 1.0f - s.p1;
    p.A = (int)s.playhead;
    p.R = (int)s.loop_start;
    p.H = s.full_range;
    p.W = (int)s.loop_end;
    p.Af = (float)p.A;
    p.Rf = (float)p.R;
    p.n = nd.n_out;
    p.k = nd.n_in - nd.n_out;
    p.nw32 = (int)s.ext_len;
    p.hist = (uint32_t*)(v.ext + s.ext_off);
    p.in_buf = v.in_buf + nd.in_off;
    p.out_buf = v.out_buf + nd.out_off;
    return true;
}
// on[] at frame g of the batch (0 <= g < K * frames)
__device__ __forceinline__ bool duck_on(const DevView& v, const DuckP& p, uint32_t g) {
    const uint32_t blk = g / (uint32_t)v.frames, f = g - blk * (uint32_t)v.frames;
    const float* pool = v.pool + (size_t)blk * v.pool_blk_stride;
    const uint8_t* fl = v.flags + (size_t)blk * v.flags_blk_stride;
    float key = 0.f;
    for (int j = 0; j < p.k; ++j) {
        const int buf = p.in_buf[p.n + j];
        if (!fl[buf]) key = fmaxf(key, fabsf(pool[(size_t)buf * v.stride + f]));  // (a NaN sample is ignored)
    }
    return key > p.T;
}
// 64 bits of the stored history from bit x0 on (x0 > -64); bits in front of the history and behind it are zero
__device__ __forceinline__ unsigned long long duck_hist64(const DuckP& p, int x0) {
    const int q = x0 >> 5, r = x0 & 31;
    const uint32_t w0 = q >= 0 && q < p.nw32 ? p.hist[q] : 0u;
    const uint32_t w1 = q + 1 >= 0 && q + 1 < p.nw32 ? p.hist[q + 1] : 0u;
    const uint32_t w2 = q + 2 >= 0 && q + 2 < p.nw32 ? p.hist[q + 2] : 0u;
    const unsigned long long lo = (unsigned long long)w0 | ((unsigned long long)w1 << 32);
    return r ? (lo >> r) | ((unsigned long long)w2 << (64 - r)) : lo;
}
// w |= w << sft over the whole bit string, in place: a word reads words below it, so the groups go from the top down
__device__ __forceinline__ void duck_shift_or(DuckLds& L, int NW, int sft, int lane) {
    const int q = sft >> 6, r = sft & 63;
    for (int r0 = ((NW - 1) / (4 * WAVE)) * (4 * WAVE); r0 >= 0; r0 -= 4 * WAVE) {
        unsigned long long a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = r0 + e * WAVE + lane, j = i - q;
            a[e] = 0ull;
            if (i < NW) {
                a[e] = L.b[i];
                if (j >= 0) a[e] |= L.b[j] << r;
                if (r && j >= 1) a[e] |= L.b[j - 1] >> (64 - r);
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = r0 + e * WAVE + lane;
            if (i < NW) L.b[i] = a[e];
        }
    }
    __syncthreads();
}
// the set bits in [lo, hi) of the staged string, 0 <= lo < hi: the same number in every lane
__device__ __forceinline__ int duck_count(const DuckLds& L, int lo, int hi, int lane) {
    const int i0 = lo >> 6, i1 = (hi - 1) >> 6;
    int cnt = 0;
    for (int i = i0 + lane; i <= i1; i += WAVE) {
        unsigned long long m = ~0ull;
        if (i == i0) m &= ~0ull << (lo & 63);
        if (i == i1) m &= ~0ull >> (63 - ((hi - 1) & 63));
        cnt += __popcll(L.b[i] & m);
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) cnt += __shfl_xor(cnt, h);
    return cnt;
}
// four bits of the staged string from bit x on (the word behind the last one used is there, and zero)
__device__ __forceinline__ uint32_t duck_bits4(const DuckLds& L, int x) {
    const int i = x >> 6, sh = x & 63;
    unsigned long long w = L.b[i] >> sh;
    if (sh > 60) w |= L.b[i + 1] << (64 - sh);
    return (uint32_t)w & 15u;
}

// run `run` of the launch's K blocks
__device__ void ducker_run(const DevView& v, const NodeDesc& nd, const DuckP& p, uint32_t run, uint32_t K, DuckLds& L) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int frames = v.frames;
    // which frames: whole blocks, about a window's worth of them so that the staged window is shared (a wave per block would read W
    // frames of key for every block), or one piece of a block longer than DUCK_RUN_MAX
    uint32_t b0, nb;
    int f_lo = 0, f_hi = frames;
    if (frames <= DUCK_RUN_MAX) {
        const int target = p.W < 256 ? 256 : (p.W > DUCK_RUN_MAX ? DUCK_RUN_MAX : p.W);
        const uint32_t bpr = target / frames > 1 ? (uint32_t)(target / frames) : 1u;
        b0 = run * bpr;
        if (b0 >= K) return;
        nb = K - b0 < bpr ? K - b0 : bpr;
    } else {
        const uint32_t ppb = (uint32_t)((frames + DUCK_RUN_MAX - 1) / DUCK_RUN_MAX);
        b0 = run / ppb;
        if (b0 >= K) return;
        nb = 1;
        f_lo = (int)(run % ppb) * DUCK_RUN_MAX;
        f_hi = frames - f_lo < DUCK_RUN_MAX ? frames : f_lo + DUCK_RUN_MAX;
    }
    const int Ln = nb == 1 ? f_hi - f_lo : (int)nb * frames;   // <= DUCK_RUN_MAX
    const int gs = (int)b0 * frames + f_lo;                     // the run's first frame, counted from the batch's
    const int Wp = (p.W + 63) & ~63;                            // bit i of the staged string is frame gs - Wp + i
    const int NW = (Wp + Ln + 63) >> 6;
    __syncthreads();  // (fwgpu_node_process takes the pieces of a long block one after the other)
    // (1) gate bits.  In front of the batch: the stored history, a word per lane
    for (int w = lane; w <= NW; w += WAVE) {
        const int g0 = gs - Wp + 64 * w;
        L.b[w] = (w < NW && g0 < 0) ? duck_hist64(p, p.W + g0) : 0ull;
    }
    __syncthreads();
    // ... from the batch's first frame on: the key buffers, a frame per lane, four words' loads in flight together
    for (int w0 = gs >= Wp ? 0 : (Wp - gs) >> 6; w0 < NW; w0 += 4) {
        unsigned long long bal[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 64 * (w0 + e) + lane, g = gs - Wp + i;
            bal[e] = __ballot(g >= 0 && i < Wp + Ln ? duck_on(v, p, (uint32_t)g) : false);
        }
        if (lane < 4 && w0 + lane < NW) L.b[w0 + lane] |= lane == 0 ? bal[0] : (lane == 1 ? bal[1] : (lane == 2 ? bal[2] : bal[3]));
    }
    __syncthreads();
    // (2) the hold: open = on dilated by H.  2^P <= H + 1 < 2^(P+1): P doublings leave the OR over 2^P frames, two of those overlapping
    // the OR over H + 1
    if (p.H > 0) {
        const int Lw = p.H + 1, P = 31 - __builtin_clz(Lw);
        for (int j = 0; j < P; ++j) duck_shift_or(L, NW, 1 << j, lane);
        if (Lw > (1 << P)) duck_shift_or(L, NW, Lw - (1 << P), lane);
    }
    // (3) the counts at the frame in front of the run (A, R <= W <= Wp: the windows are staged)
    int ca = duck_count(L, Wp - p.A, Wp, lane), cr = duck_count(L, Wp - p.R, Wp, lane);
    // (4) block by block, 256 frames at a time, four consecutive frames per lane
    int pos = Wp;
    for (uint32_t ib = 0; ib < nb; ++ib) {
        const uint32_t blk = b0 + ib;
        float* pool = v.pool + (size_t)blk * v.pool_blk_stride;
        uint8_t* fl = v.flags + (size_t)blk * v.flags_blk_stride;
        const uint64_t silent = __ballot(lane < p.n ? fl[p.in_buf[lane]] != 0 : false);
        for (int cf = f_lo; cf < f_hi; cf += 4 * WAVE) {
            const int f0 = cf + 4 * lane;
            const int valid = f_hi - f0 >= 4 ? 4 : (f_hi - f0 > 0 ? f_hi - f0 : 0);
            const uint32_t vm = (1u << valid) - 1u;
            const int x = pos + (f0 - f_lo);
            uint32_t en = 0u, la = 0u, lr = 0u;
            if (valid) {
                en = duck_bits4(L, x) & vm;          // frames that enter both windows
                la = duck_bits4(L, x - p.A) & vm;    // ... that leave the A-window
                lr = duck_bits4(L, x - p.R) & vm;    // ... and the R-window
            }
            // inclusive scan of the three counts (each at most 256: ten bits apiece)
            const uint32_t own = (uint32_t)__popc(en) | ((uint32_t)__popc(la) << 10) | ((uint32_t)__popc(lr) << 20);
            uint32_t inc = own;
#pragma unroll
            for (int h = 1; h < WAVE; h <<= 1) {
                const uint32_t t = __shfl_up(inc, h);
                if (lane >= h) inc += t;
            }
            const uint32_t exc = inc - own, tot = __shfl(inc, WAVE - 1);
            v4f g;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t m = (2u << e) - 1u;
                const int in_ = (int)(exc & 1023u) + __popc(en & m);
                const int cae = ca + in_ - (int)((exc >> 10) & 1023u) - __popc(la & m);
                const int cre = cr + in_ - (int)(exc >> 20) - __popc(lr & m);
                const float a = (float)cae / p.Af;
                const float r = (float)cre / p.Rf;
                const float u = fmaxf(a, r);
                g[e] = 1.0f - (p.dd * u);
            }
            if (valid)
                for (int c = 0; c < p.n; ++c) {
                    float* out = pool + (size_t)p.out_buf[c] * v.stride + f0;
                    v4f y = splat(0.f);  // (a main channel flagged silent is not read: zeros out, flagged)
                    if (!((silent >> c) & 1ull)) {
                        const v4f xin = __builtin_nontemporal_load((const v4f*)(pool + (size_t)p.in_buf[c] * v.stride + f0));
                        y = xin * g;
                    }
                    __builtin_nontemporal_store(y, (v4f*)out);
                }
            ca += (int)(tot & 1023u) - (int)((tot >> 10) & 1023u);
            cr += (int)(tot & 1023u) - (int)(tot >> 20);
        }
        pos += f_hi - f_lo;
        // the meter's pass-through rule for the main channels; nothing else is ever flagged
        if (lane < p.n) fl[p.out_buf[lane]] = (silent >> lane) & 1ull ? 1 : 0;
    }
}

// the history a launch of K blocks leaves behind: new[i] = S[i + K * frames], S = old history ++ the batch's gate bits.  A shift of the
// slice in place where the batch is shorter than W: groups of 64 words go up, every load of a group is back before its first store.
__device__ void ducker_history(const DevView& v, const DuckP& p, uint32_t K) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long total = (long long)K * v.frames;
    const int nw64 = p.nw32 >> 1;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (int t0 = 0; t0 < nw64; t0 += WAVE) {
        const int t = t0 + lane;
        const long long x0 = 64ll * t + total;  // where word t of the new history starts in S
        unsigned long long hv = (t < nw64 && x0 < p.W) ? duck_hist64(p, (int)x0) : 0ull;
        const int t1 = nw64 - t0 < WAVE ? nw64 - t0 : WAVE;
        for (int e0 = 0; e0 < t1; e0 += 4) {
            unsigned long long bal[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 64 * (t0 + e0 + e) + lane;  // bit of the new history
                const long long x = (long long)i + total;
                bal[e] = __ballot(i < p.W && x >= p.W ? duck_on(v, p, (uint32_t)(x - p.W)) : false);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (lane == e0 + e) hv |= bal[e];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);  // (vmcnt(0): the loaded words are in registers)
        if (t < nw64) {
            p.hist[2 * t] = (uint32_t)hv;
            p.hist[2 * t + 1] = (uint32_t)(hv >> 32);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// one workgroup of one wave per (node of the level, run); nodes of other kinds are k_level's.  own_hist: the launch is one run, and its
// wave writes the history back itself
__global__ __launch_bounds__(WAVE) void k_ducker(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K, int own_hist) {
    __shared__ DuckLds L;
    if ((int)blockIdx.x >= n_nodes) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_DUCKER) return;
    DuckP p;
    if (!duck_params(v, nd, v.states[nd.state], p)) return;
    ducker_run(v, nd, p, blockIdx.y, K, L);
    if (own_hist && blockIdx.y == 0) ducker_history(v, p, K);
}
// the follow-up of a launch of more than one run: one wave per node
__global__ __launch_bounds__(WAVE) void k_ducker_hist(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K) {
    if ((int)blockIdx.x >= n_nodes) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_DUCKER) return;
    DuckP p;
    if (!duck_params(v, nd, v.states[nd.state], p)) return;
    ducker_history(v, p, K);
}
