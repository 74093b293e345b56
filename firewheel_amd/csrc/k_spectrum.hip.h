// k_spectrum.hip.h — SPEC spectrum meter (K_METER created with two or more parameters): per (block, input channel) the band
// powers of a Hann-windowed N-point FFT over the channel's last N frames.  A kernel of its own behind k_level<0>, which renders the
// node as the level meter it also is (pass-through audio, flags, level records); included by fwgpu_kernels.hip.
//
// Per channel, x[n] the frames since activation (x[n < 0] = +0.0; a block flagged silent counts as +0.0 and is not read), block g with
// last frame n_g, all in f32, every operation rounded, no FMA:
//   v[i] = x[n_g - N + 1 + i] * w[i];  re[i] = v[bitrev(i)], im[i] = +0.0;
//   stages h = 1, 2, .., N/2, groups of 2h, j < h: a = element j, b = element j + h, k = j * (N / 2h),
//       tr = (wr[k]*b.re) - (wi[k]*b.im), ti = (wr[k]*b.im) + (wi[k]*b.re), a' = a + t, b' = a - t;
//   P[k] = ((re[k]*re[k]) + (im[k]*im[k])) * (16 / N^2), k = 0..N/2;  band b = ((P[e[b]] + P[e[b]+1]) + ..) + P[e[b+1]-1].
// w, wr, wi and e are the host's tables in the node's slice (fwgpu_types.h spec_*): no sinf / cosf here.
//
// No recurrence in time: a block is a function of the N frames that end with it.  One workgroup of SPEC_THREADS takes one (node, block,
// channel) of a launch of K blocks of `frames` frames each.  With g = (b + 1) * frames - N + i the position of window frame i of block b
// counted from the launch's first frame, the source of the frame is, as in k_delay_comp,
//   g >= 0: frame g % frames of the INPUT of block g / frames of the launch (this block's or an earlier one's; that block's flag holds);
//   g <  0: the stored history hist[c][N + g] (the last N input frames in front of the launch, oldest first).
// The N complex values and the twiddles live in LDS, 4-byte words, index i at word i + i / 64: the bit-reversed store of the window
// puts a wave's 64 values N / 64 words apart — at N = 4096 all in one of the 64 banks — and the pad spreads them over all 64; the
// stages' own strides (2 at h = 1, 1 from h = 64 on) meet at most two ways.
// More than one workgroup of a launch reads the history, so none of them writes it: k_spectrum_hist, a workgroup per node launched right
// behind k_spectrum (stream order is the barrier), stores the last N frames of (history ++ the launch).  A launch of one block writes
// them itself: its workgroups each own one channel.

#define SPEC_THREADS 256
#define SPEC_IDX(i) ((i) + ((i) >> 6))

struct SpecLds {
    float re[SPEC_FFT_MAX + SPEC_FFT_MAX / 64];
    float im[SPEC_FFT_MAX + SPEC_FFT_MAX / 64];
    float wr[SPEC_FFT_MAX / 2 + SPEC_FFT_MAX / 128];
    float wi[SPEC_FFT_MAX / 2 + SPEC_FFT_MAX / 128];
};
// what one workgroup knows about its node
struct SpecP {
    int N, logN, B, n;
    uint32_t R;
    const float* win;       // w[N]
    const float* tw;        // wr[N/2] wi[N/2]
    const uint32_t* edges;  // e[B + 1]
    float* hist;            // hist[n][N]
    float* ring;            // [R][n][B]
    const int* in_buf;
};
// false: a plain meter, or state a plan build would not let through (a slice of another size would be indexed out of bounds)
__device__ __forceinline__ bool spec_params(const DevView& v, const NodeDesc& nd, const NodeState& s, SpecP& p) {
    if (!spec_on(s) || !spec_state_ok(s, nd.n_in, nd.n_out) || s.ext_len != spec_ext_len(s, nd.n_in) || v.frames < 1 || v.frames > v.stride) return false;
    p.N = (int)s.loop_start;
    p.logN = 31 - __builtin_clz((unsigned)p.N);
    p.B = s.playing;
    p.n = nd.n_in;
    p.R = (uint32_t)s.loop_end;
    float* slice = v.ext + s.ext_off;
    p.win = slice + spec_win_rel(s, nd.n_in);
    p.tw = slice + spec_tw_rel(s, nd.n_in);
    p.edges = (const uint32_t*)(slice + spec_edges_rel(s, nd.n_in));
    p.hist = slice + spec_hist_rel(s, nd.n_in);
    p.ring = slice + spec_ring_rel(s, nd.n_in);
    p.in_buf = v.in_buf + nd.in_off;
    return true;
}

// block b of the launch, channel c: the record goes to rec[0..B)
__device__ void spec_block(const DevView& v, const SpecP& p, uint32_t b, int c, float* rec, SpecLds& L) {
    const int t = threadIdx.x;
    const int N = p.N, F = v.frames, half = N >> 1;
    const int buf = p.in_buf[c];
    for (int k = t; k < half; k += SPEC_THREADS) {
        L.wr[SPEC_IDX(k)] = p.tw[k];
        L.wi[SPEC_IDX(k)] = p.tw[half + k];
    }
    const long long g0 = (long long)(b + 1u) * F - N;
    const float* hist = p.hist + (size_t)c * N;
    for (int i = t; i < N; i += SPEC_THREADS) {
        const long long g = g0 + i;
        float x = 0.f;
        if (g < 0) {
            x = hist[N + g];  // (g >= frames - N)
        } else {
            const uint32_t sb = (uint32_t)g / (uint32_t)F, off = (uint32_t)g - sb * (uint32_t)F;  // (sb <= b)
            if (v.flags[(size_t)sb * v.flags_blk_stride + buf] == 0) x = v.pool[(size_t)sb * v.pool_blk_stride + (size_t)buf * v.stride + off];
        }
        const int r = (int)(__brev((unsigned)i) >> (32 - p.logN));
        L.re[SPEC_IDX(r)] = x * p.win[i];
        L.im[SPEC_IDX(r)] = 0.f;
    }
    __syncthreads();
    for (int lh = 0; lh < p.logN; ++lh) {
        const int h = 1 << lh;
        for (int q = t; q < half; q += SPEC_THREADS) {
            const int j = q & (h - 1);
            const int ia = SPEC_IDX(((q - j) << 1) | j), ib = SPEC_IDX((((q - j) << 1) | j) + h), ik = SPEC_IDX(j << (p.logN - 1 - lh));
            const float wr = L.wr[ik], wi = L.wi[ik];
            const float ar = L.re[ia], ai = L.im[ia], br = L.re[ib], bi = L.im[ib];
            const float tr = (wr * br) - (wi * bi);
            const float ti = (wr * bi) + (wi * br);
            L.re[ia] = ar + tr;
            L.im[ia] = ai + ti;
            L.re[ib] = ar - tr;
            L.im[ib] = ai - ti;
        }
        __syncthreads();
    }
    // the powers take the place of the imaginary parts: a thread reads and writes its own bins only
    const float scale = 16.0f / ((float)N * (float)N);  // (a power of two)
    for (int k = t; k <= half; k += SPEC_THREADS) {
        const float re = L.re[SPEC_IDX(k)], im = L.im[SPEC_IDX(k)];
        L.im[SPEC_IDX(k)] = ((re * re) + (im * im)) * scale;
    }
    __syncthreads();
    for (int bnd = t; bnd < p.B; bnd += SPEC_THREADS) {
        const int e0 = (int)p.edges[bnd];
        int e1 = (int)p.edges[bnd + 1];
        if (e1 > half + 1) e1 = half + 1;  // (the host's edges end at N/2 + 1)
        float sum = 0.f;
        if (e0 >= 0 && e0 < e1) {
            sum = L.im[SPEC_IDX(e0)];
            for (int k = e0 + 1; k < e1; ++k) sum = sum + L.im[SPEC_IDX(k)];
        }
        rec[bnd] = sum;
    }
}

// what a launch of K blocks leaves behind for channel c: new[i] = S[i + K * frames], S = the old history ++ the launch's input (flagged
// blocks as zeros).  A shift in place where the launch is shorter than N: groups of SPEC_THREADS go up, every load of a group is back
// before the group's first store, and no group reads what an earlier one wrote.  (Every thread of the workgroup makes every trip.)
__device__ void spec_history(const DevView& v, const SpecP& p, int c, uint32_t K) {
    const int t = threadIdx.x;
    const int N = p.N, F = v.frames;
    const long long total = (long long)K * F;
    const int buf = p.in_buf[c];
    float* hist = p.hist + (size_t)c * N;
    for (int i0 = 0; i0 < N; i0 += SPEC_THREADS) {  // (N is a multiple of SPEC_THREADS)
        const int i = i0 + t;
        const long long s = (long long)i + total;
        float x = 0.f;
        if (s < N) {
            x = hist[s];
        } else {
            const uint32_t g = (uint32_t)(s - N), blk = g / (uint32_t)F, f = g - blk * (uint32_t)F;  // (blk < K)
            if (v.flags[(size_t)blk * v.flags_blk_stride + buf] == 0) x = v.pool[(size_t)blk * v.pool_blk_stride + (size_t)buf * v.stride + f];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);  // (vmcnt(0): the loaded values are in registers)
        __syncthreads();
        hist[i] = x;
    }
}

// one workgroup per (node of the level, block, channel); nodes that are no spectrum meters return at once.  own_hist: the launch is one
// block, and the workgroup of a channel writes that channel's history back itself
__global__ __launch_bounds__(SPEC_THREADS) void k_spectrum(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K, int own_hist) {
    if ((int)blockIdx.x >= n_nodes || blockIdx.y >= K) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_METER || nd.state < 0 || (int)blockIdx.z >= nd.n_in) return;
    SpecP p;
    if (!spec_params(v, nd, v.states[nd.state], p)) return;
    __shared__ SpecLds L;
    const uint32_t b = blockIdx.y;
    const int c = (int)blockIdx.z;
    // the meter's slot rule: a launch longer than the ring keeps its last R blocks
    if (v.meter_K - b <= p.R) spec_block(v, p, b, c, p.ring + ((size_t)((v.meter_blk0 + b) % p.R) * (size_t)p.n + (size_t)c) * (size_t)p.B, L);
    if (own_hist && b == 0) spec_history(v, p, c, K);
}
// the follow-up of a launch of more than one block: one workgroup per node
__global__ __launch_bounds__(SPEC_THREADS) void k_spectrum_hist(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K) {
    if ((int)blockIdx.x >= n_nodes) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_METER || nd.state < 0) return;
    SpecP p;
    if (!spec_params(v, nd, v.states[nd.state], p)) return;
    for (int c = 0; c < p.n; ++c) spec_history(v, p, c, K);
}
