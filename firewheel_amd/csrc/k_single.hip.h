// k_single.hip.h — B1: one node on scratch buffers (fwgpu_node_process), a single wave.  Included by fwgpu_kernels.hip last of the node
// kernels: it runs every node kind, k_level's and the four that bring a kernel of their own.
// A limiter, a ducker, a latency-compensation delay or a compressor renders one block through its stored history, which the call leaves
// advanced; one node never needs two kinds' LDS, and the delay needs none
// SPM: the build for a spatialiser (launch_single_node: DevView::sp_moves) — it takes CMD_SP_MOVE and renders a move; every other kind
// runs the build without it
// GR: the build for a volume or a pan (DevView::gain_rides) — it takes CMD_GAIN_RIDE and renders a ride
template <bool SPM, bool GR = false>
__global__ __launch_bounds__(WAVE) void k_single_node(DevView v, int node_idx) {
    __shared__ union {
        LimLds lim;
        DuckLds duck;
        CompLds comp;
    } lds;
    const int kind = v.nodes[node_idx].kind;
    if (kind == K_LIMITER) {
        limiter_node(v, v.nodes[node_idx], 0, 1, lds.lim);
        return;
    }
    if (kind == K_DUCKER) {
        const NodeDesc nd = v.nodes[node_idx];
        DuckP p;
        if (!duck_params(v, nd, v.states[nd.state], p)) return;
        const uint32_t pieces = v.frames > DUCK_RUN_MAX ? (uint32_t)((v.frames + DUCK_RUN_MAX - 1) / DUCK_RUN_MAX) : 1u;
        for (uint32_t run = 0; run < pieces; ++run) ducker_run(v, nd, p, run, 1, lds.duck);
        ducker_history(v, p, 1);
        return;
    }
    if (kind == K_COMPRESSOR) {
        const NodeDesc nd = v.nodes[node_idx];
        CompP p;
        if (!comp_params(v, nd, v.states[nd.state], p)) return;
        const uint32_t pieces = v.frames > COMP_RUN_MAX ? (uint32_t)((v.frames + COMP_RUN_MAX - 1) / COMP_RUN_MAX) : 1u;
        for (uint32_t run = 0; run < pieces; ++run) compressor_run(v, p, run, 1, lds.comp);
        compressor_history(v, p, 1);
        return;
    }
    if (kind == K_DELAY_COMP) {
        const NodeDesc nd = v.nodes[node_idx];
        DcompP p;
        if (!dcomp_params(v, nd, v.states[nd.state], p)) return;
        dcomp_block(v, p, 0);
        dcomp_history(v, p, 1);
        return;
    }
    node_process_wave<3, SPM, GR>(v, node_idx, 0, 0);
}
