// k_delay_comp.hip.h — SPEC latency compensation (K_DELAY_COMP): a pure delay of D whole frames, a kernel of its own next
// to k_level, as k_limiter and k_ducker are.  Included by fwgpu_kernels.hip; it needs no LDS.
//
// Per channel c and frame n since activation (x_c[n < 0] = +0.0; a channel flagged silent for a block counts as +0.0 for that block and
// is not read):  y_c[n] = x_c[n - D] — a copy, no arithmetic: -0.0, infinities, subnormals and NaN payloads keep their bits.
// Silence: one counter loud_c per channel, 0 at activation.  Output channel c of a block of F frames is zero-filled and flagged iff its
// input is flagged for this block and loud_c == 0 in front of the block; behind the block loud_c = D if the input was not flagged,
// max(0, loud_c - F) otherwise.
//
// No recurrence in time: a block is a function of the D frames in front of it and its own input.  One wave takes one (node, block) of a
// launch of K blocks of `frames` frames each, whatever D and `frames` are.  With g = b * frames + p - D the position of output frame p of
// block b counted from the batch's first frame, the source of the frame is
//   g >= 0: frame g % frames of the INPUT of block g / frames of the batch — this block's own or an earlier one's, pool - j *
//           pool_blk_stride, which the level above has written for the whole batch (as k_ducker reads its key); that block's flag holds;
//   g <  0: the node's stored history hist[c][D + g] (the last D input frames in front of the batch, oldest first).
// The counter a block sees follows from the stored one and the flags of the blocks in front of it in the batch: the nearest block whose
// input was not flagged, at most ceil(D / frames) blocks back, searched 64 blocks per step with one ballot.
// Loads are dwords, the four of a lane all issued before its 16-byte store (channel buffers are 256-byte aligned, a lane's quad starts
// at a multiple of four frames).
// More than one wave of a launch reads the stored history and the counters, so none of them writes either: k_delay_comp_hist, a wave
// per node launched right behind k_delay_comp (stream order is the barrier), stores the last D frames of (history ++ the batch) and the
// counters.  A launch that one wave renders whole (K = 1; fwgpu_node_process) writes them itself.

// what one wave knows about its node
struct DcompP {
    int D, n;
    float* hist;       // hist[n][D]
    uint32_t* loud;    // loud[n], behind the history
    const int* in_buf;
    const int* out_buf;
};
// false: state a plan build would not let through — the host harness holds it to that (a slice of another size would be indexed out
// of bounds)
__device__ __forceinline__ bool dcomp_params(const DevView& v, const NodeDesc& nd, const NodeState& s, DcompP& p) {
    if (!dcomp_state_ok(s, nd.n_in, nd.n_out) || s.ext_len != dcomp_ext_len(s, nd.n_in) || v.frames < 1 || v.frames > v.stride) return false;
    p.D = (int)s.loop_start;
    p.n = nd.n_in;
    p.hist = v.ext + s.ext_off;
    p.loud = (uint32_t*)(p.hist + (size_t)p.n * p.D);
    p.in_buf = v.in_buf + nd.in_off;
    p.out_buf = v.out_buf + nd.out_off;
    return true;
}
// loud_c in front of block b of the batch (b = K: behind the batch), for the channel that reads pool buffer `buf`: the same number in
// every lane.  `stored`: the counter in front of the batch.
__device__ __forceinline__ int dcomp_loud(const DevView& v, const DcompP& p, int buf, uint32_t stored, uint32_t b) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int F = v.frames;
    if (p.D == 0) return 0;
    const uint32_t reach = (uint32_t)((p.D + F - 1) / F);  // after this many flagged blocks nothing is left of any counter
    const uint32_t look = b < reach ? b : reach;
    for (uint32_t j0 = 0; j0 < look; j0 += WAVE) {
        const uint32_t j = j0 + (uint32_t)lane;  // block b - 1 - j
        const bool heard = j < look && v.flags[(size_t)(b - 1u - j) * v.flags_blk_stride + buf] == 0;
        const uint64_t m = __ballot(heard);
        if (m) return p.D - (int)(j0 + (uint32_t)__builtin_ctzll(m)) * F;  // (j < reach: positive)
    }
    if (b < reach) {  // every block of the batch in front of b was flagged
        const long long left = (long long)stored - (long long)b * F;
        return left > 0 ? (int)left : 0;
    }
    return 0;
}

// block b of the launch
__device__ void dcomp_block(const DevView& v, const DcompP& p, uint32_t b) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int F = v.frames, D = p.D;
    float* pool = v.pool + (size_t)b * v.pool_blk_stride;
    uint8_t* fl = v.flags + (size_t)b * v.flags_blk_stride;
    uint32_t quiet = 0u;  // bit c: output channel c is zero-filled and flagged
    for (int c = 0; c < p.n; ++c) {
        const int buf = p.in_buf[c];
        if (fl[buf] != 0 && dcomp_loud(v, p, buf, p.loud[c], b) == 0) quiet |= 1u << c;
    }
    for (int cf = 0; cf < F; cf += 4 * WAVE) {
        const int f0 = cf + 4 * lane;
        if (f0 >= F) continue;
        // where the four frames come from, the same for every channel: a block of the batch (sb >= 0) and a frame in it, the stored
        // history (sb == -1) and an index into it, or nothing (sb == -2: the frame lies behind the block's last one)
        int sb[4], so[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int g = (int)b * F + f0 + e - D;
            if (f0 + e >= F) {
                sb[e] = -2;
                so[e] = 0;
            } else if (g < 0) {
                sb[e] = -1;
                so[e] = D + g;  // (g >= -D)
            } else {
                sb[e] = (int)((uint32_t)g / (uint32_t)F);  // (<= b)
                so[e] = g - sb[e] * F;
            }
        }
        for (int c = 0; c < p.n; ++c) {
            v4f y = splat(0.f);
            if (!((quiet >> c) & 1u)) {
                const int buf = p.in_buf[c];
                const float* src[4];
                bool live[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    src[e] = p.hist;
                    live[e] = false;
                    if (sb[e] == -1) {
                        src[e] = p.hist + (size_t)c * D + so[e];
                        live[e] = true;
                    } else if (sb[e] >= 0) {  // (a block flagged silent counts as +0.0 and is not read)
                        src[e] = v.pool + (size_t)sb[e] * v.pool_blk_stride + (size_t)buf * v.stride + so[e];
                        live[e] = v.flags[(size_t)sb[e] * v.flags_blk_stride + buf] == 0;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = live[e] ? *src[e] : 0.f;
            }
            *(v4f*)(pool + (size_t)p.out_buf[c] * v.stride + f0) = y;  // (f0 + 3 < stride: a multiple of 64 that is >= frames)
        }
    }
    if (lane < p.n) fl[p.out_buf[lane]] = (quiet >> lane) & 1u ? 1 : 0;
}

// what a launch of K blocks leaves behind: new[c][i] = S_c[i + K * frames], S_c = the old history ++ the batch's input (flagged blocks as
// zeros), and the counters behind the last block.  A shift of the slice in place where the batch is shorter than D: groups of 256 go up,
// every load of a group is back before the group's first store, and no group reads what an earlier one wrote.
__device__ void dcomp_history(const DevView& v, const DcompP& p, uint32_t K) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int F = v.frames, D = p.D;
    const long long total = (long long)K * F;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (int c = 0; c < p.n; ++c) {
        const int buf = p.in_buf[c];
        const int left = dcomp_loud(v, p, buf, p.loud[c], K);
        float* hist = p.hist + (size_t)c * D;
        for (int i0 = 0; i0 < D; i0 += 4 * WAVE) {
            float x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + e * WAVE + lane;
                x[e] = 0.f;
                if (i < D) {
                    const long long s = (long long)i + total;
                    if (s < D) {
                        x[e] = hist[s];
                    } else {
                        const uint32_t g = (uint32_t)(s - D), blk = g / (uint32_t)F, f = g - blk * (uint32_t)F;  // (blk < K)
                        if (v.flags[(size_t)blk * v.flags_blk_stride + buf] == 0)
                            x[e] = v.pool[(size_t)blk * v.pool_blk_stride + (size_t)buf * v.stride + f];
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);  // (vmcnt(0): the loaded values are in registers)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + e * WAVE + lane;
                if (i < D) hist[i] = x[e];
            }
        }
        if (lane == 0) p.loud[c] = (uint32_t)left;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// one workgroup of one wave per (node of the level, block); nodes of other kinds are k_level's.  own_hist: the launch is one block, and
// its wave writes the history back itself
__global__ __launch_bounds__(WAVE) void k_delay_comp(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K, int own_hist) {
    if ((int)blockIdx.x >= n_nodes || blockIdx.y >= K) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_DELAY_COMP) return;
    DcompP p;
    if (!dcomp_params(v, nd, v.states[nd.state], p)) return;
    dcomp_block(v, p, blockIdx.y);
    if (own_hist && blockIdx.y == 0) dcomp_history(v, p, K);
}
// the follow-up of a launch of more than one block: one wave per node
__global__ __launch_bounds__(WAVE) void k_delay_comp_hist(DevView v, const int* __restrict__ level_nodes, int n_nodes, uint32_t K) {
    if ((int)blockIdx.x >= n_nodes) return;
    const NodeDesc nd = v.nodes[level_nodes[blockIdx.x]];
    if (nd.kind != K_DELAY_COMP) return;
    DcompP p;
    if (!dcomp_params(v, nd, v.states[nd.state], p)) return;
    dcomp_history(v, p, K);
}
