// k_limiter.hip.h — SPEC look-ahead limiter (K_LIMITER): a kernel of its own next to k_level, as k_bus_iir is, so that
// its LDS (the staged target gains of a chunk) and its registers are paid by no other node kind.  Included by fwgpu_kernels.hip.
//
// Per frame n since activation (x[n < 0] = +0.0, a channel flagged silent counts as +0.0):
//   key[n] = max_c |x_c[n]| (fmaxf from +0.0)        t[n] = key[n] > C ? C / key[n] : 1.0f   (IEEE division)
//   m[n]   = min t[n-63-H .. n]                       s[n] = ((m[n-63] + m[n-62]) + ...) + m[n]   (64 terms, ascending, no FMA)
//   g[n]   = s[n] * 0.015625f                         y_c[n] = x_c[n-63] * g[n]
// No recurrence in time: a block is a function of the H + 126 frames in front of it and its own input.  One wave renders a block in
// chunks of 256 frames:  (1) t for the chunk's 256 + 126 + H positions into LDS;  (2) the sliding minimum by doubling in place —
// a[k] = min(a[k], a[k + 2^j]) for j = 0 .. P-1 leaves min t[k .. k + 2^P) with 2^P <= 64 + H < 2^(P+1), and the window of 64 + H is two
// of those overlapping (a minimum is exact: any order gives the same bits);  (3) lane l runs the 64-add chains of frames l, l + 64,
// l + 128, l + 192 of the chunk from LDS — consecutive lanes read consecutive words, no bank conflict — scales, multiplies the delayed
// input and stores, 256 contiguous bytes per wave instruction.
//
// Where the frames in front of a block come from: the node's ext slice hist[n_in][HK], HK = H + 128, oldest first (block 0 of a launch,
// and every block of the serial path), or — parallel path, K > 1 blocks of at least H + 126 frames — the tail of block b-1's INPUT,
// which the level above has already written for the whole batch (as a frozen spatialiser reads it).  On the parallel path the block-0
// wave, the only one that reads the slice, stores the history the batch leaves behind after its own block (spatial_finish's pattern).
#define LIM_CHUNK 256
#define LIM_BACK (2 * (LIM_LOOK - 1))                      // frames in front of an output frame that its gain depends on, without H
#define LIM_T_WORDS (LIM_CHUNK + LIM_BACK + LIM_HOLD_MAX + 2)  // 2304
#define LIM_M_WORDS (LIM_CHUNK + LIM_LOOK)                 // 320: m for the chunk and the 63 frames in front of it
struct LimLds {
    float t[LIM_T_WORDS];
    float m[LIM_M_WORDS];
};

// what one wave knows about its node and block
struct LimIO {
    const float* pool;     // this block's pool slice
    const float* prev;     // the slice of the block before (parallel path), or nullptr: the frames in front come from `hist`
    const float* hist;     // hist[n_in][HK]
    const int* in_buf;
    uint64_t silent, prev_silent;  // in-masks of this block and of the one before
    int stride, frames, HK;
    // x_c[p], p in [-HK, frames) relative to the block's first frame
    __device__ __forceinline__ float x(int c, int p) const {
        if (p >= 0) return ((silent >> c) & 1ull) ? 0.f : pool[(size_t)in_buf[c] * stride + p];
        if (prev) return ((prev_silent >> c) & 1ull) ? 0.f : prev[(size_t)in_buf[c] * stride + frames + p];
        return hist[(size_t)c * HK + HK + p];
    }
};
__device__ __forceinline__ LimIO lim_io(const DevView& v, const NodeDesc& nd, const NodeState& s, uint32_t blk, bool from_prev) {
    const int lane = threadIdx.x & (WAVE - 1);
    LimIO io;
    io.pool = v.pool + (size_t)blk * v.pool_blk_stride;
    io.prev = from_prev ? io.pool - v.pool_blk_stride : nullptr;
    io.hist = v.ext + s.ext_off;
    io.in_buf = v.in_buf + nd.in_off;
    io.stride = v.stride;
    io.frames = v.frames;
    io.HK = (int)s.loop_end;
    const uint8_t* fl = v.flags + (size_t)blk * v.flags_blk_stride;
    io.silent = __ballot(lane < nd.n_in ? fl[io.in_buf[lane]] != 0 : false);
    io.prev_silent = __ballot(from_prev && lane < nd.n_in ? (fl - v.flags_blk_stride)[io.in_buf[lane]] != 0 : false);
    return io;
}

// one block of the node, by one wave
__device__ void limiter_block(const DevView& v, const NodeDesc& nd, const NodeState& s, uint32_t blk, bool from_prev, LimLds& L) {
    const int lane = threadIdx.x & (WAVE - 1);
    const LimIO io = lim_io(v, nd, s, blk, from_prev);
    const int n_ch = nd.n_in, frames = v.frames;
    const int H = (int)s.loop_start;
    const float C = s.p0;
    const int Lw = LIM_LOOK + H;            // the minimum's window
    const int P = 31 - __builtin_clz(Lw);   // 2^P <= Lw < 2^(P+1)
    const int* out_buf = v.out_buf + nd.out_off;
    float* out_pool = v.pool + (size_t)blk * v.pool_blk_stride;
    for (int base = 0; base < frames; base += LIM_CHUNK) {
        const int cn = frames - base < LIM_CHUNK ? frames - base : LIM_CHUNK;
        const int W = cn + LIM_BACK + H;     // staged positions: t[i] belongs to frame p0 + i
        const int Q = cn + LIM_LOOK - 1;     // m[q] belongs to frame base - 63 + q; its window starts at t[q]
        const int p0 = base - LIM_BACK - H;
        for (int i = lane; i < W; i += WAVE) {
            float key = 0.f;
            for (int c = 0; c < n_ch; ++c) key = fmaxf(key, fabsf(io.x(c, p0 + i)));  // (a NaN sample is ignored)
            L.t[i] = key > C ? C / key : 1.0f;
        }
        __syncthreads();
        for (int j = 0; j < P; ++j) {
            const int sft = 1 << j;
            for (int r0 = 0; r0 < W; r0 += 4 * WAVE) {  // reads of a group of rows before its writes; later rows are not written yet
                float a[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = r0 + e * WAVE + lane;
                    a[e] = 1.0f;
                    if (k < W) a[e] = k + sft < W ? fminf(L.t[k], L.t[k + sft]) : L.t[k];
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = r0 + e * WAVE + lane;
                    if (k < W) L.t[k] = a[e];
                }
            }
            __syncthreads();
        }
        const int second = Lw - (1 << P);  // [q, q + Lw) = [q, q + 2^P) u [q + second, q + second + 2^P)
        for (int q = lane; q < Q; q += WAVE) L.m[q] = fminf(L.t[q], L.t[q + second]);
        __syncthreads();
        float acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = L.m[lane + e * WAVE];  // (words past Q are read and never used: inside the array)
#pragma unroll 7
        for (int k = 1; k < LIM_LOOK; ++k) {  // (63 = 9 x 7; unrolled in full, the loads of all 252 words are hoisted: 254 VGPRs)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] + L.m[lane + e * WAVE + k];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = lane + e * WAVE;
            if (j >= cn) continue;
            const float g = acc[e] * 0.015625f;
            const int f = base + j;
            for (int c = 0; c < n_ch; ++c) (out_pool + (size_t)out_buf[c] * v.stride)[f] = io.x(c, f - (LIM_LOOK - 1)) * g;
        }
        __syncthreads();  // (the next chunk overwrites t and m)
    }
    // what goes out is never flagged silent (a filter's outputs are not either)
    if (lane < nd.n_out) (v.flags + (size_t)blk * v.flags_blk_stride)[out_buf[lane]] = 0;
}

// the history block `blk` leaves behind: the last HK frames of (what was in front of it ++ its input).  Where that is a shift of the
// slice in place, reads run ahead of writes: every load of a group of 256 is back before the group's first store.
__device__ void limiter_history(const DevView& v, const NodeDesc& nd, const NodeState& s, uint32_t blk, bool from_prev) {
    const int lane = threadIdx.x & (WAVE - 1);
    const LimIO io = lim_io(v, nd, s, blk, from_prev);
    const int HK = io.HK;
    float* hist = v.ext + s.ext_off;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (int c = 0; c < nd.n_in; ++c)
        for (int i0 = 0; i0 < HK; i0 += 4 * WAVE) {
            float x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + e * WAVE + lane;
                x[e] = i < HK ? io.x(c, i - HK + io.frames) : 0.f;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);  // (vmcnt(0): the loaded values are in registers)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + e * WAVE + lane;
                if (i < HK) hist[(size_t)c * HK + i] = x[e];
            }
        }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // (the serial path reads the slice again for the next block)
}

// block b of a launch of K blocks.  Parallel path: every block has at least H + 126 frames, so block b > 0 finds all it needs in block
// b-1's input.  Otherwise (short blocks, a one-block launch) the b == 0 wave takes the K blocks in order through the stored history.
// (L: the caller's LDS — k_limiter's own, or k_single_node's, which a ducker shares)
__device__ void limiter_node(const DevView& v, const NodeDesc& nd, uint32_t b, uint32_t K, LimLds& L) {
    const NodeState& s = v.states[nd.state];
    const uint64_t H = s.loop_start;
    // (nothing a plan build lets through — the host harness holds it to that; a slice of another size would be indexed out of bounds)
    if (!lim_state_ok(s, nd.n_in, nd.n_out) || s.ext_len != lim_ext_len(s, nd.n_in) || v.frames < 1) return;
    if (K > 1 && (uint64_t)v.frames >= H + LIM_BACK) {
        limiter_block(v, nd, s, b, b > 0, L);
        if (b == 0) limiter_history(v, nd, s, K - 1, true);
    } else if (b == 0) {
        for (uint32_t blk = 0; blk < K; ++blk) {
            limiter_block(v, nd, s, blk, false, L);
            limiter_history(v, nd, s, blk, false);
        }
    }
}

// one workgroup of one wave per (node of the level, block); nodes of other kinds are k_level's
__global__ __launch_bounds__(WAVE) void k_limiter(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K) {
    __shared__ LimLds L;
    if ((int)blockIdx.x >= n_nodes) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_LIMITER) return;
    limiter_node(v, nd, blockIdx.y, K, L);
}
