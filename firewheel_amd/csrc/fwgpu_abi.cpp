// fwgpu_abi.cpp — the C ABI of include/fwgpu.h: device counterpart of FirewheelGraphCtx + FirewheelProcessor
// (graph/context.rs, graph/processor.rs).  The host half keeps the editable graph, the device half keeps node state,
// the buffer pool and the launch plan in HBM.  No CPU compute path exists: every process call is kernels.
#include "fwgpu_ctx.h"

#include <chrono>
#include <memory>
#include <stdio.h>

namespace {

// hipSetDevice costs ~8 us per call on this stack (measured: it was most of the host time of a realtime callback); the
// thread's current device is asked first, which is a thread-local read
inline void use_device(fwgpu_ctx* c) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != c->device) (void)hipSetDevice(c->device);
}

thread_local std::string g_create_error;  // fwgpu_create_error(): of the calling thread's last failed fwgpu_ctx_create

// Control side of a message: validate against the graph (owned by the control side), account for the sampler's ring
// capacity, then hand the message to the lock-free ring.  May run while the audio thread is inside a process call.
int push_cmd(fwgpu_ctx* c, int64_t node, int want_kind, Cmd m, bool counts_as_msg) {
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (want_kind >= 0 && n->kind != want_kind) return fail(c, FWGPU_ERR_INVALID, "node kind does not accept this message");
    if (counts_as_msg) {  // sampler.rs:14 CHANNEL_CAPACITY messages between two drains of the ring
        const uint64_t ep = c->drain_epoch.load(std::memory_order_acquire);
        if (n->pending_epoch != ep) {
            n->pending_epoch = ep;
            n->pending_msgs = 0;
        }
        if (n->pending_msgs >= 128) return fail(c, FWGPU_ERR_QUEUE_FULL, "sampler message ring full");
    }
    m.state = (int)(node & 0xffffffff);
    if (!n->activated) {
        // no built plan holds this node yet (add_node, then a message, then fwgpu_update — the reference's ring simply waits
        // for the processor's first block): the message is released when the plan that activates it is published, so that a
        // process call running on the OLD plan neither consumes it nor applies it to a stale slot.  Control side, like update.
        if (c->early_msgs.size() >= fwgpu_ctx::RING_CAP) return fail(c, FWGPU_ERR_QUEUE_FULL, "too many messages for nodes that are not activated yet");
        c->early_msgs.push_back(m);
        if (counts_as_msg) n->pending_msgs++;
        return 0;
    }
    if (!c->ring.push(m)) return fail(c, FWGPU_ERR_QUEUE_FULL, "context message ring full (no process call is draining it)");
    if (counts_as_msg) n->pending_msgs++;
    return 0;
}

void rebuild_sample_table(fwgpu_ctx* c) {  // control side: host copy of the device sample table
    c->h_sample_tab.resize(std::max<size_t>(c->samples.size(), 1));
    if (c->samples.empty()) memset(&c->h_sample_tab[0], 0, sizeof(SampleDesc));
    for (size_t i = 0; i < c->samples.size(); ++i) c->h_sample_tab[i] = c->samples[i].desc;
    c->samples_dirty = true;  // copied to the device by the next process / update call
}

// swapped-out samples whose process call has completed on the device: RetRing -> ret_ready, reference counts updated
void collect_returns(fwgpu_ctx* c) {
    RetItem it;
    while (c->returns.peek(it)) {
        // tickets are issued in call order: an unfinished call ends the scan.  An event slot that has been re-recorded
        // since (64 calls with returns later) answers for the later call — later, never earlier, than the truth.
        if (it.ticket >= c->ret_done_ticket.load(std::memory_order_acquire)) {
            const uint32_t slot = it.ticket % fwgpu_ctx::RET_EVENTS;
            if (c->ret_event_ticket[slot].load(std::memory_order_acquire) <= it.ticket) break;  // not recorded for this call yet
            if (hipEventQuery(c->ret_events[slot]) != hipSuccess) {
                (void)hipGetLastError();
                break;
            }
        }
        c->returns.pop();
        if (it.sample >= 0 && (size_t)it.sample < c->sample_refs.size() && c->sample_refs[it.sample] > 0) c->sample_refs[it.sample]--;
        if (it.node != RET_SILENT) c->ret_ready.push_back(it);
    }
}

// ---- SPEC streaming sources, control side
size_t stream_elem_size(int fmt) { return (fmt == FMT_I_F32 || fmt == FMT_P_F32) ? 4 : 2; }
StreamRec* stream_of(fwgpu_ctx* c, int sample) {
    if (sample < 0 || sample >= (int)c->samples.size() || !c->samples[sample].alive) return nullptr;
    const int si = c->samples[sample].stream;
    return si >= 0 && si < (int)c->streams.size() ? &c->streams[si] : nullptr;
}
// the audio side stops publishing the stream's sampler (under the gate: the audio side reads the table inside its calls)
void stream_pub_drop(fwgpu_ctx* c, StreamRec& r) {
    if (r.pub < 0) return;
    ControlGate gate(c);
    c->stream_pub_slot[r.pub] = -1;
    c->stream_pub_n--;
    r.pub = -1;
}
// the sampler let go of the stream (another sample, the node removed, the stream destroyed): finished for good
void stream_detach(fwgpu_ctx* c, StreamRec& r) {
    stream_pub_drop(c, r);
    r.detached = true;
    r.finished = true;
}
// C, U and `finished` of every bound stream as of the last process call KNOWN to be complete: the newest bank whose event has
// completed and whose ticket did not move while it was read.  Never blocks.
void stream_refresh(fwgpu_ctx* c) {
    if (!c->h_stream_pub || c->stream_pub_n == 0) return;
    const uint64_t t0 = c->stream_pub_ticket[0].load(std::memory_order_acquire), t1 = c->stream_pub_ticket[1].load(std::memory_order_acquire);
    const int order[2] = {t0 >= t1 ? 0 : 1, t0 >= t1 ? 1 : 0};
    for (int k = 0; k < 2; ++k) {
        const int bank = order[k];
        const uint64_t t = c->stream_pub_ticket[bank].load(std::memory_order_acquire);
        if (!t) continue;
        if (hipEventQuery(c->ev_stream_pub[bank]) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        bool torn = false;
        for (StreamRec& r : c->streams) {
            if (r.pub < 0) continue;
            NodeState st;
            memcpy(&st, c->h_stream_pub + (size_t)bank * fwgpu_ctx::STREAM_PUB_MAX + r.pub, sizeof(st));
            if (c->stream_pub_ticket[bank].load(std::memory_order_acquire) != t) {
                torn = true;
                break;
            }
            if (st.sample != r.sample || !smp_stream_on(st)) continue;  // (the bind message has not been applied yet)
            const SmpStream ss = smp_stream_of(st);
            if (ss.C >= r.consumed) {  // (counts only move forward: an older bank never overrides a newer one)
                r.consumed = ss.C;
                r.starved = ss.U;
                if (ss.flags & SMP_STREAM_FINISHED) r.finished = true;
            }
        }
        if (!torn) break;
    }
    // a finished stream has nothing left to publish: the resident realtime kernel may come back
    for (StreamRec& r : c->streams)
        if (r.pub >= 0 && r.finished) stream_pub_drop(c, r);
}
uint64_t stream_free(const StreamRec& r) { return r.ring - (r.written - r.consumed); }
// `frames` frames at ring position written % R, split at the ring's end and, planar, per channel: src laid out as a sample of
// `src_frames` frames (null: zero padding — bytes of 0, or 0x8000 elements for the unsigned formats).  Plain copies on the control side's stream,
// waited for on that stream alone
int stream_put(fwgpu_ctx* c, const StreamRec& r, const void* src, uint64_t frames, uint64_t src_frames, bool on_device) {
    const SampleDesc& d = c->samples[r.sample].desc;
    const size_t es = stream_elem_size(d.format), ch = (size_t)d.channels;
    const bool planar = d.format >= FMT_P_I16;
    const uint64_t pos = r.written % r.ring;
    const uint64_t n0 = std::min<uint64_t>(frames, r.ring - pos), n1 = frames - n0;
    std::vector<uint16_t> pad;
    if (!src && (d.format == FMT_I_U16 || d.format == FMT_P_U16)) {
        pad.assign((size_t)frames * ch, (uint16_t)0x8000);
        src = pad.data();
        on_device = false;
    }
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    auto piece = [&](uint64_t dst_elem, uint64_t src_elem, uint64_t elems) -> hipError_t {
        if (!elems) return hipSuccess;
        char* dst = (char*)d.data + dst_elem * es;
        if (!src) return hipMemsetAsync(dst, 0, elems * es, c->stream_wr);
        return hipMemcpyAsync(dst, (const char*)src + src_elem * es, elems * es, kind, c->stream_wr);
    };
    hipError_t e = hipSuccess;
    if (planar) {
        for (size_t k = 0; k < ch && e == hipSuccess; ++k) {
            e = piece(k * r.ring + pos, k * src_frames, n0);
            if (e == hipSuccess) e = piece(k * r.ring, k * src_frames + n0, n1);
        }
    } else {
        e = piece(pos * ch, 0, n0 * ch);
        if (e == hipSuccess) e = piece(0, n0 * ch, n1 * ch);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream_wr);  // the data has landed before the sampler is told of it
    return e == hipSuccess ? 0 : hipfail(c, e, "stream write");
}
// one CMD_SMP_STREAM to the bound sampler, at_block 0: the new W and, with has_end, E
int stream_tell(fwgpu_ctx* c, StreamRec& r, uint64_t W, bool has_end, uint64_t E) {
    if (r.node < 0 || r.detached) return 0;
    return push_cmd(c, r.node, K_SAMPLER, make_smp_stream(W, has_end, E), true);
}

}  // namespace

// ================================================================= C ABI
extern "C" {

// every entry point that takes a context: a null handle is an error return, never a crash
#define NEED_CTX(c, ret) \
    do {                 \
        if (!(c)) return (ret); \
    } while (0)

const char* fwgpu_create_error(void) { return g_create_error.c_str(); }

fwgpu_ctx* fwgpu_ctx_create(int device, uint32_t sample_rate, uint32_t max_block_frames, uint32_t num_graph_inputs,
                            uint32_t num_graph_outputs, void* hip_stream) {
    g_create_error.clear();
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e) +
                         " (libfwgpu has no CPU fallback)";
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        g_create_error = "device index out of range";
        return nullptr;
    }
    if (max_block_frames == 0 || num_graph_inputs > 64 || num_graph_outputs > 64) {
        g_create_error = "invalid arguments (max_block_frames > 0, <= 64 graph channels)";
        return nullptr;
    }
    if ((e = hipSetDevice(device)) != hipSuccess) {
        g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return nullptr;
    }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) {
        g_create_error = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return nullptr;
    }
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        g_create_error = std::string("device is ") + prop.gcnArchName + "; libfwgpu ships gfx950 (MI355X) code only";
        return nullptr;
    }
    fwgpu_ctx* c = new fwgpu_ctx(num_graph_inputs, num_graph_outputs);
    c->graph.limbo = &c->limbo_slots;  // a removed node's slot is reused only once no running plan holds the node
    c->device = device;
    c->sample_rate = sample_rate;
    c->mbf = max_block_frames;
    c->stride = (int)((max_block_frames + 63) / 64 * 64);
    c->n_gin = num_graph_inputs;
    c->n_gout = num_graph_outputs;
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
            g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e);
            delete c;
            return nullptr;
        }
        c->own_stream = true;
    }
    // message path: every buffer gets its final size here (a process call never allocates for messages)
    {
        bool ok = c->ring.init(fwgpu_ctx::RING_CAP) && c->returns.init(4096);
        c->cmds.reserve(fwgpu_ctx::CMD_CAP);
        c->cmds_scratch.reserve(fwgpu_ctx::CMD_CAP);
        c->ret_ready.reserve(4096);
        ok = ok && c->d_cmds.ensure_n("d_cmds", fwgpu_ctx::CMD_CAP * sizeof(Cmd)) == hipSuccess;
        ok = ok && hipHostMalloc((void**)&c->h_cmds, fwgpu_ctx::CMD_CAP * sizeof(Cmd), hipHostMallocDefault) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->cmds_copied, hipEventDisableTiming) == hipSuccess;
        for (uint32_t i = 0; ok && i < fwgpu_ctx::RET_EVENTS; ++i)
            ok = hipEventCreateWithFlags(&c->ret_events[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            g_create_error = "message ring / staging allocation failed";
            fwgpu_ctx_destroy(c);
            return nullptr;
        }
    }
    rebuild_sample_table(c);
    {
        std::vector<float> tab(RS_PHASES * RS_TAPS);
        resampler_table(tab.data());
        if (upload(c, c->d_rs_table, tab.data(), tab.size() * sizeof(float)) != 0) {
            g_create_error = c->err_ctl;
            fwgpu_ctx_destroy(c);
            return nullptr;
        }
    }
    if (upload_sample_table(c) != 0 || c->d_mask.ensure_n("d_mask", 64) != hipSuccess) {
        g_create_error = c->err_ctl;
        fwgpu_ctx_destroy(c);
        return nullptr;
    }
    // realtime I/O blocks: allocated here, on the control thread (the process calls never allocate).  A failure is not
    // fatal: process_interleaved then always takes the staged-copy path.
    if (hipHostMalloc((void**)&c->h_rt_in, RT_IO_BYTES, hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void**)&c->h_rt_out, RT_IO_BYTES, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->d_rt_in, c->h_rt_in, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->d_rt_out, c->h_rt_out, 0) != hipSuccess) {
        if (c->h_rt_in) (void)hipHostFree(c->h_rt_in);
        if (c->h_rt_out) (void)hipHostFree(c->h_rt_out);
        c->h_rt_in = c->h_rt_out = nullptr;
        (void)hipGetLastError();
    }
    if (hipHostMalloc((void**)&c->h_rt_flag, 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->d_rt_flag, c->h_rt_flag, 0) != hipSuccess) {
        if (c->h_rt_flag) (void)hipHostFree(c->h_rt_flag);
        c->h_rt_flag = c->d_rt_flag = nullptr;
        (void)hipGetLastError();
    } else {
        *c->h_rt_flag = 0;
    }
    if (const char* e = getenv("FWGPU_RT_SPIN")) {
        if (atoi(e) == 0 && c->h_rt_flag) {  // experiments: blocking stream sync instead of the polled completion flag
            (void)hipHostFree(c->h_rt_flag);
            c->h_rt_flag = c->d_rt_flag = nullptr;
        }
    }
    if (const char* e = getenv("FWGPU_CTL_AHEAD")) {
        c->ctl_ahead = atoi(e) != 0;
        if (atoi(e) == 1) c->ctl_ahead_mode = 1;
    }
    if (c->ctl_ahead) {  // its own high-priority stream + the events that order it against the render stream
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        bool ok = hipStreamCreateWithPriority(&c->ctl_stream, hipStreamNonBlocking, hi) == hipSuccess;
        for (int i = 0; ok && i < 2; ++i)
            ok = hipEventCreateWithFlags(&c->ev_ctl[i], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&c->ev_render[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            c->ctl_ahead = false;
        }
    }
    if (const char* e = getenv("FWGPU_LAZY")) c->lazy_on = atoi(e) != 0;
    if (c->lazy_on) {  // the control kernels' horizon word + where it is published for the host (fwgpu_types.h LazyRec)
        bool ok = c->d_lazy_horizon.ensure_n("d_lazy_horizon", 256) == hipSuccess && hipMemset(c->d_lazy_horizon.p, 0xff, 256) == hipSuccess &&
                  hipHostMalloc((void**)&c->h_lazy_pub, 64, hipHostMallocMapped) == hipSuccess &&
                  hipHostGetDevicePointer((void**)&c->d_lazy_pub, c->h_lazy_pub, 0) == hipSuccess;
        if (ok) {
            memset(c->h_lazy_pub, 0, 64);
        } else {
            (void)hipGetLastError();
            c->lazy_on = false;
        }
    }
    if (const char* e = getenv("FWGPU_LEAF_GROUP")) c->group_on = atoi(e) != 0;
    if (const char* e = getenv("FWGPU_LEAF_GROUP_MIN")) c->group_min_items = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("FWGPU_RT_PERSIST")) c->rt_persist = atoi(e) != 0;
    if (const char* e = getenv("FWGPU_LEVEL_FUSE")) c->level_fuse = atoi(e) != 0;
    if (const char* e = getenv("FWGPU_GATE_DEFER_US")) c->gate_defer_ns = (uint64_t)std::max(0, atoi(e)) * 1000ull;
    if (const char* e = getenv("FWGPU_RT_IDLE_MS")) c->rt_idle_ms = (uint32_t)std::max(1, atoi(e));
    const bool quiet_given = getenv("FWGPU_QUIET_WAIT_US") != nullptr;
    if (const char* e = getenv("FWGPU_QUIET_WAIT_US")) c->quiet_wait_us = (uint32_t)std::max(0, atoi(e));
    if (const char* e = getenv("FWGPU_UP_DIFF")) c->up_diff = atoi(e) != 0;
    if (const char* e = getenv("FWGPU_BUILD_ONE_KERNEL")) c->build_one_kernel = atoi(e) != 0;
    if (const char* e = getenv("FWGPU_BUILD_STREAM")) c->build_on_audio_stream = strcmp(e, "own") != 0;
    // a group in the AUDIO stream queues behind whatever callback is in flight and costs the next one its own few microseconds wherever it
    // lands: beside back-to-back callbacks the 100 us a group used to wait for a window that never comes were 0.2 ms of every edit
    // (fw_edit_race, same box: typical edit 1.13 -> 0.96 ms, same p99).  On its own stream a group still waits the longer time.
    if (!quiet_given && !c->build_on_audio_stream) c->quiet_wait_us = 100;
    if (const char* e = getenv("FWGPU_UP_PIECE")) c->up_piece = (uint32_t)std::max(4096, atoi(e));
    if (c->rt_persist && c->h_rt_flag) {  // mailbox in pinned, device-mapped host memory + the kernel's own (non-blocking) stream
        bool ok = hipHostMalloc((void**)&c->h_rt_mb, sizeof(RtMailbox), hipHostMallocMapped) == hipSuccess &&
                  hipHostGetDevicePointer((void**)&c->d_rt_mb, c->h_rt_mb, 0) == hipSuccess;
        if (ok) memset(c->h_rt_mb, 0, sizeof(RtMailbox));
        // HIGH priority, not for the priority: ROCm multiplexes a process's streams onto a few hardware queues PER PRIORITY LEVEL, and
        // whatever shares a queue with a kernel that never ends waits behind it — a plain hipMemcpy of a control thread (the null
        // stream) sat out the whole 4 s of a fed resident kernel (r04, tests/test_rt_resident.py).  The high-priority pool holds
        // only this stream and ctl_stream, which is never used while a resident kernel runs (throughput calls end it first).
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        ok = ok && hipStreamCreateWithPriority(&c->rt_stream, hipStreamNonBlocking, hi) == hipSuccess &&
             hipEventCreateWithFlags(&c->rt_ev, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            c->rt_persist = false;
        }
    } else {
        c->rt_persist = false;
    }
    if (const char* e = getenv("FWGPU_HOST_PROF")) c->host_prof = atoi(e) != 0;
    if (const char* e = getenv("FWGPU_PLAN_ORDER")) c->graph.canonical_order = strcmp(e, "reference") != 0;
    if (const char* e = getenv("FWGPU_UPDATE_PROF")) {
        c->update_prof = atoi(e) != 0;
        c->update_prof_tables = atoi(e) >= 2;
    }
    if (const char* e = getenv("FWGPU_RT_GRAPH")) c->rt_use_graph = atoi(e) != 0;
    if (const char* e = getenv("FWGPU_RT_ONE_LAUNCH")) c->rt_one_launch = atoi(e) != 0;
    if (const char* e = getenv("FWGPU_RT_PERSIST_MAX_LEAVES")) c->rt_persist_max_leaves = std::max(0, atoi(e));
    if (c->d_rt_sync.ensure_n("d_rt_sync", 256) != hipSuccess || hipMemset(c->d_rt_sync.p, 0, 256) != hipSuccess) c->d_rt_sync.release();
    return c;
}

void fwgpu_ctx_destroy(fwgpu_ctx* c) {
    if (!c) return;
    if (c->host_prof && c->hp_calls)
        fprintf(stderr, "fwgpu host profile: %llu process calls, %.2f us each inside run_blocks; %llu k_rt_block launches, %.2f us each inside the HIP launch call\n",
                (unsigned long long)c->hp_calls, c->hp_call_ns / 1e3 / (double)c->hp_calls, (unsigned long long)c->hp_launches,
                c->hp_launches ? c->hp_launch_ns / 1e3 / (double)c->hp_launches : 0.0);
    if (c->host_prof && c->hp_calls) {
        fprintf(stderr, "fwgpu host profile: host time inside run_blocks, 25 us bins:");
        for (int i = 0; i < 16; ++i) fprintf(stderr, " %llu", (unsigned long long)c->hp_hist[i]);
        fprintf(stderr, "\n");
    }
    if (c->update_prof && c->phase_updates > 1) {
        const double n = (double)(c->phase_updates - 1);
        fprintf(stderr, "fwgpu update profile: %.0f updates after the first; mean us per phase (fwgpu_update_phase):", n);
        for (int i = 1; i < 32; ++i)
            if (c->phase_ns[i]) fprintf(stderr, " [%d] %.1f", i, c->phase_ns[i] / 1e3 / n);
        fprintf(stderr, "; per update: %.1f launches of k_build_apply, %.1f jobs, %.1f KiB copied, %.1f KiB filled\n", c->prof_groups / n, c->prof_jobs / n,
                c->prof_copy_bytes / 1024.0 / n, c->prof_fill_bytes / 1024.0 / n);
    }
    use_device(c);
    (void)rt_persist_stop(c);
    // (in the default output mode the graph-output kernel writes the mapped host staging below FROM c->stream; a ctx
    //  destroyed with a begun, un-ended ticket must not unregister / free it under a kernel that is still storing into it)
    (void)hipStreamSynchronize(c->stream);
    if (c->rt_stream) (void)hipStreamDestroy(c->rt_stream);
    if (c->rt_ev) (void)hipEventDestroy(c->rt_ev);
    if (c->ao.copy_stream) {
        (void)hipStreamSynchronize(c->ao.copy_stream);
        (void)hipStreamDestroy(c->ao.copy_stream);
    }
    if (c->host_prof && c->ao.prof_calls)
        fprintf(stderr, "fwgpu host profile: %llu process_interleaved_end calls: %.1f us waiting for the copy back, %.1f us in memcpy each\n",
                (unsigned long long)c->ao.prof_calls, c->ao.prof_wait_ns / 1e3 / (double)c->ao.prof_calls, c->ao.prof_copy_ns / 1e3 / (double)c->ao.prof_calls);
    for (int i = 0; i < 2; ++i) {
        if (c->ao.ev_render[i]) (void)hipEventDestroy(c->ao.ev_render[i]);
        if (c->ao.ev_copy[i]) (void)hipEventDestroy(c->ao.ev_copy[i]);
        if (c->ao.h[i]) {
            (void)hipHostUnregister(c->ao.h[i]);
            free(c->ao.h[i]);
        }
        c->ao.d[i].release();
    }
    if (c->h_rt_mb) (void)hipHostFree(c->h_rt_mb);
    if (c->h_lazy_pub) (void)hipHostFree(c->h_lazy_pub);
    (void)hipStreamSynchronize(c->stream);
    if (c->ctl_stream) {
        (void)hipStreamSynchronize(c->ctl_stream);
        (void)hipStreamDestroy(c->ctl_stream);
    }
    for (hipEvent_t e : {c->ev_ctl[0], c->ev_ctl[1], c->ev_render[0], c->ev_render[1], c->ev_join})
        if (e) (void)hipEventDestroy(e);
    for (SampleRec& s : c->samples)
        if (s.alive && s.owned && s.d_data) (void)hipFree(s.d_data);
    // plan images: the active one (this ctx's base), a published one nobody adopted, the spare, whatever the ring still holds
    if (PlanImage* p = c->pending.exchange(nullptr)) {
        p->release_device();
        delete p;
    }
    if (c->spare) {
        c->spare->release_device();
        delete c->spare;
    }
    for (uint32_t h = c->retired_head.load(); h != c->retired_tail.load(); ++h) {
        PlanImage* p = c->retired[h % fwgpu_ctx::RETIRE_CAP];
        p->release_device();
        delete p;
    }
    c->release_device();
    if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
    if (c->h_up) (void)hipHostFree(c->h_up);
    if (c->h_jobs) (void)hipHostFree(c->h_jobs);
    if (c->ev_build) (void)hipEventDestroy(c->ev_build);
    if (c->stream_wr) (void)hipStreamDestroy(c->stream_wr);
    if (c->h_stream_pub) (void)hipHostFree(c->h_stream_pub);
    if (c->h_stream_jobs) (void)hipHostFree(c->h_stream_jobs);
    for (hipEvent_t e : c->ev_stream_pub)
        if (e) (void)hipEventDestroy(e);
    DevBuf* bufs[] = {&c->d_states, &c->d_ext, &c->d_samples, &c->d_rt_sync, &c->d_lazy_horizon, &c->d_cmds, &c->d_in_stage, &c->d_out_stage, &c->d_scratch_pool,
                      &c->d_scratch_flags, &c->d_scratch_tab, &c->d_mask, &c->d_trace, &c->d_rs_table, &c->d_fir_stats};
    for (DevBuf* b : bufs) b->release();
    for (TimerCat& t : c->timers)
        for (auto& p : t.ev) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    if (c->h_rt_in) (void)hipHostFree(c->h_rt_in);
    if (c->h_rt_out) (void)hipHostFree(c->h_rt_out);
    if (c->h_rt_flag) (void)hipHostFree(c->h_rt_flag);
    if (c->h_cmds) (void)hipHostFree(c->h_cmds);
    if (c->cmds_copied) (void)hipEventDestroy(c->cmds_copied);
    for (hipEvent_t e : c->ret_events)
        if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* fwgpu_last_error(fwgpu_ctx* c) {
    if (!c) return "null ctx";
    return c->err_last.load(std::memory_order_acquire) ? c->err_audio : c->err_ctl;
}

int64_t fwgpu_graph_in_node(fwgpu_ctx* c) { return c ? c->graph.id_of(c->graph.graph_in_slot) : FWGPU_ERR_INVALID; }
int64_t fwgpu_graph_out_node(fwgpu_ctx* c) { return c ? c->graph.id_of(c->graph.graph_out_slot) : FWGPU_ERR_INVALID; }

int64_t fwgpu_add_node(fwgpu_ctx* c, int kind, uint32_t n_in, uint32_t n_out, const float* params, int n_params) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (kind < 0 || kind > K_KIND_MAX) return fail(c, FWGPU_ERR_INVALID, "unsupported node kind");
    if (n_params < 0 || (n_params > 0 && !params)) return fail(c, FWGPU_ERR_INVALID, "params is null but n_params > 0");
    if (kind == K_FIR || kind == K_RESAMPLER) {
        int ir = n_params > 0 ? (int)params[0] : -1;
        if (ir < 0 || ir >= (int)c->samples.size() || !c->samples[ir].alive || c->samples[ir].desc.frames == 0)
            return fail(c, FWGPU_ERR_INVALID, kind == K_FIR ? "FIR node: params[0] must be the id of a non-empty impulse-response sample"
                                                            : "Resampler node: params[0] must be the id of a non-empty source sample");
        if (c->samples[ir].stream >= 0)
            return fail(c, FWGPU_ERR_INVALID, "a stream cannot be an impulse response or a resampler's source");
        if (kind == K_FIR && c->samples[ir].desc.frames > (1u << 24))
            return fail(c, FWGPU_ERR_INVALID, "FIR node: at most 2^24 taps");
        if (kind == K_RESAMPLER && c->samples[ir].desc.frames >= (1ull << 31))
            return fail(c, FWGPU_ERR_INVALID, "Resampler node: source longer than 2^31 frames");
    }
    if (n_in > 64 || n_out > 64) return fail(c, FWGPU_ERR_INVALID, "a node has at most 64 ports per side (core/node.rs:62,69)");
    if (kind_has_own_kernel(kind) || kind == K_CROSSFADE) {  // (its shape is refused here; its creation parameters at the next update, as a meter's ring is)
        std::string err;
        if (!check_activation(kind, n_in, n_out, err)) return fail(c, FWGPU_ERR_INVALID, err);
    }
    NodeState st = make_state(kind, params, n_params, c->sample_rate);
    const int64_t id = c->graph.add_node(kind, n_in, n_out, st);
    if (kind == K_FIR && n_params >= 2 && id >= 0)  // SPEC FIR morph: two or more parameters make the node morph-capable
        if (HostNode* hn = c->graph.get(id)) {
            hn->fir_morph = true;
            hn->fir_ir[0] = st.sample;
            hn->fir_ir[1] = st.s1.status;
            hn->fir_max_taps = fw_bits_of(st.s1.a);
            hn->fir_target = st.p1;
            hn->fir_target_end = 0;
        }
    return id;
}
// control side: `sample` has lost a FIR user (a node removed, a slot exchanged) — each of its converted copies (one per channel and
// padded length T) that no FIR node of that T, and none that waits for its activation, uses any more goes to limbo until the first image built without it is the
// active one
static void fir_ir_release(fwgpu_ctx* c, int sample) {
    if (sample < 0) return;
    for (auto it = c->ir_cache.begin(); it != c->ir_cache.end();) {
        bool used = false;
        if (std::get<0>(it->first) == sample)
            for (const HostNode& n : c->graph.nodes)  // (a node that waits for its activation may need any length: it keeps the copies)
                if (fir_uses_sample(n, sample) && (!n.activated || n.init.loop_start == std::get<2>(it->first))) used = true;
        if (std::get<0>(it->first) == sample && !used) {
            c->limbo.push_back({c->build_gen + 1, 1, it->second, (uint32_t)(((size_t)std::get<2>(it->first) + 63) / 64 * 64)});
            it = c->ir_cache.erase(it);
        } else {
            ++it;
        }
    }
}
int fwgpu_remove_node(fwgpu_ctx* c, int64_t node) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    // the node's slice of the ext state pool (delay rings, FIR history, biquad / spatialiser state) goes back to a free
    // list keyed by size; the next activation of a node that needs the same amount reuses it, zeroed (install_plan) —
    // a host that spawns and retires effect voices does not grow HBM without bound
    struct Freed {
        bool any = false, activated = false;
        uint32_t off = 0, len = 0;
        int kind = 0, ir = -1, ir_b = -1;
    } fr;
    if (HostNode* hn = c->graph.get(node))
        if (hn->activated) {
            fr.activated = true;
            fr.any = hn->init.ext_len != 0;
            fr.off = hn->init.ext_off;
            fr.len = hn->init.ext_len;
            fr.ir = hn->kind == K_FIR ? (hn->fir_morph ? hn->fir_ir[0] : hn->init.sample) : -1;
            fr.ir_b = hn->kind == K_FIR && hn->fir_morph ? hn->fir_ir[1] : -1;
        }
    if (HostNode* hn = c->graph.get(node)) fr.kind = hn->kind;
    int held_stream = -1;  // (SPEC streaming source: removing the sampler leaves its stream finished)
    if (HostNode* hn = c->graph.get(node)) held_stream = hn->stream;
    int rc = c->graph.remove_node(node);
    if (rc == 0 && held_stream >= 0 && held_stream < (int)c->streams.size()) stream_detach(c, c->streams[held_stream]);
    if (rc) return fail(c, rc, "remove_node: unknown node or graph in/out node");
    if (fr.any) c->limbo.push_back({c->build_gen + 1, 1, fr.off, (uint32_t)(((size_t)fr.len + 63) / 64 * 64)});
    fir_ir_release(c, fr.ir);  // the f32 copies of an impulse response go with its last FIR user (either slot)
    if (fr.ir_b != fr.ir) fir_ir_release(c, fr.ir_b);
    // The node is gone from the GRAPH; the running plan may hold it until the next plan is adopted.  What it still owns —
    // its slot (the message key), its ext slice, messages queued for it, a sampler's sample — is released AT that adoption
    // (adopt_image) or after it (release_limbo), never from this thread while a process call may be using it.
    const uint32_t slot = (uint32_t)(node & 0xffffffff);
    const uint64_t tag = c->build_gen + 1;  // the first image built without the node
    for (uint32_t sl : c->limbo_slots) c->limbo.push_back({tag, 0, sl, 0});
    c->limbo_slots.clear();
    if (fr.activated) c->pending_removed.push_back(slot);
    {  // (messages that never left the control side)
        size_t w = 0;
        for (const Cmd& m : c->early_msgs) {
            if (m.state == (int)slot) {
                const int smp = m.type == CMD_SMP_SET_SAMPLE ? smp_cmd_sample(m) : -1;
                if (smp >= 0 && (size_t)smp < c->sample_refs.size() && c->sample_refs[smp] > 0) c->sample_refs[smp]--;
                continue;
            }
            c->early_msgs[w++] = m;
        }
        c->early_msgs.resize(w);
    }
    if (fr.kind == K_SAMPLER && fr.activated) c->dropped_samplers_ctl.push_back(slot);  // Drop: sampler.rs:563-571
    return 0;
}
int64_t fwgpu_connect(fwgpu_ctx* c, int64_t src, uint32_t sp, int64_t dst, uint32_t dp, int check) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    return c->graph.connect(src, sp, dst, dp, check != 0);
}
int fwgpu_disconnect(fwgpu_ctx* c, int64_t src, uint32_t sp, int64_t dst, uint32_t dp) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    return c->graph.disconnect(src, sp, dst, dp);
}
int fwgpu_disconnect_edge(fwgpu_ctx* c, int64_t e) { return c ? c->graph.disconnect_edge(e) : FWGPU_ERR_INVALID; }
int fwgpu_cycle_detected(fwgpu_ctx* c) { return c ? (c->graph.cycle_detected() ? 1 : 0) : FWGPU_ERR_INVALID; }

// ---- latency queries (include/fwgpu.h, "latency compensation"): pure host code over the current edge set
int fwgpu_node_latency(fwgpu_ctx* c, int64_t node, uint32_t* frames) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    const HostNode* hn = c->graph.get(node);
    if (!hn) return fail(c, FWGPU_ERR_INVALID, "node_latency: unknown node");
    if (frames) *frames = HostGraph::own_latency(*hn);
    return 0;
}
int64_t fwgpu_graph_latency_report(fwgpu_ctx* c, fwgpu_latency_skew* out, uint32_t cap) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (cap && !out) return fail(c, FWGPU_ERR_INVALID, "latency_report: out is null but cap > 0");
    const HostGraph& g = c->graph;
    std::vector<uint32_t> lat;
    if (!g.arrival_latency(lat)) return fail(c, FWGPU_ERR_COMPILE_CYCLE, "cycle detected");
    int64_t total = 0;
    for (uint32_t slot = 0; slot < g.nodes.size(); ++slot) {
        const HostNode& n = g.nodes[slot];
        if (!n.alive) continue;
        uint32_t latest = 0;
        for (uint32_t p = 0; p < n.n_in; ++p)
            if (n.in_edge[p] >= 0) latest = std::max(latest, lat[g.edges[n.in_edge[p]].src]);
        for (uint32_t p = 0; p < n.n_in; ++p) {
            if (n.in_edge[p] < 0) continue;
            const uint32_t arrives = lat[g.edges[n.in_edge[p]].src];
            if (arrives == latest) continue;
            if ((uint64_t)total < cap) out[total] = fwgpu_latency_skew{g.id_of(slot), p, latest - arrives};
            total++;
        }
    }
    return total;
}
int fwgpu_graph_output_latency(fwgpu_ctx* c, uint32_t* frames) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    std::vector<uint32_t> lat;
    if (!c->graph.arrival_latency(lat)) return fail(c, FWGPU_ERR_COMPILE_CYCLE, "cycle detected");
    if (frames) *frames = lat[c->graph.graph_out_slot];  // (graph_out adds nothing of its own)
    return 0;
}

int fwgpu_host_node_set_process(fwgpu_ctx* c, int64_t node, fwgpu_host_process_fn fn, void* user) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* hn = c->graph.get(node);
    if (!hn || hn->kind != K_HOST) return fail(c, FWGPU_ERR_INVALID, "not a host node (fwgpu_add_node with FWGPU_HOST_NODE)");
    if (!fn) return fail(c, FWGPU_ERR_INVALID, "host node: null process function");
    const size_t slot = (size_t)(node & 0xffffffff);
    if (c->host_procs.size() <= slot) c->host_procs.resize(std::max<size_t>(slot + 1, c->host_procs.size() * 2));
    c->host_procs[slot].fn = fn;
    c->host_procs[slot].user = user;
    c->graph.needs_compile = true;  // the plan holds a copy of the function pointer: the next update installs the new one
    return 0;
}
int fwgpu_plan_host_nodes(fwgpu_ctx* c, uint64_t* callbacks_run) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (callbacks_run) *callbacks_run = c->host_callbacks;  // (of the active image: meaningful once the audio side is quiet)
    return c->info.have_plan ? c->info.n_host_nodes : -1;
}

// which part of fwgpu_update the control thread is in (include/fwgpu.h): read by any thread, written by the updating one
int fwgpu_update_phase(fwgpu_ctx* c) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    return c->update_phase.load(std::memory_order_relaxed);
}
int fwgpu_update(fwgpu_ctx* c) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    use_device(c);
    if (!c->graph.needs_compile && c->info.have_plan) return 0;
    Plan plan = std::move(c->spare_plan);  // (the node array of the image recycled by the last build: control side only)
    c->spare_plan = Plan();
    std::string err;
    phase_mark(c, 1);
    int rc = c->graph.build_plan(plan, err);
    if (rc) {
        phase_mark(c, 0);
        return fail(c, rc, err);
    }
    phase_mark(c, 2);
    {
        RtHold hold(c);  // table growth frees device memory (hipFree waits for every stream): no resident realtime kernel meanwhile
        rc = install_plan(c, plan);
    }
    phase_mark(c, 0);
    return rc;
}

int fwgpu_schedule_upload(fwgpu_ctx* c, const fwgpu_sched_node* sn, uint32_t n_nodes, uint32_t num_buffers) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    use_device(c);
    if (n_nodes < 2 || !sn) return fail(c, FWGPU_ERR_INVALID, "a schedule holds at least graph_in and graph_out");
    for (uint32_t i = 0; i < n_nodes; ++i)
        if ((sn[i].num_inputs && (!sn[i].in_buffer_index || !sn[i].in_should_clear)) || (sn[i].num_outputs && !sn[i].out_buffer_index))
            return fail(c, FWGPU_ERR_INVALID, "schedule node with ports but null buffer tables");
    Plan plan;
    std::vector<std::pair<int, int>> last_writer(num_buffers, std::make_pair(-1, 0));
    std::vector<char> seen(c->graph.nodes.size(), 0);  // a node runs once per block (schedule.rs:289-344): two entries for one
                                                       // node would be two waves read-modify-writing one NodeState
    for (uint32_t i = 0; i < n_nodes; ++i) {
        HostNode* hn = c->graph.get(sn[i].node);
        if (!hn) return fail(c, FWGPU_ERR_INVALID, "schedule names an unknown node");
        {
            const uint32_t slot = (uint32_t)(sn[i].node & 0xffffffff);
            if (seen[slot]) return fail(c, FWGPU_ERR_INVALID, "schedule names a node twice");
            seen[slot] = 1;
            const bool io = slot == c->graph.graph_in_slot || slot == c->graph.graph_out_slot;
            if (io && i != 0 && i != n_nodes - 1)
                return fail(c, FWGPU_ERR_INVALID, "graph_in / graph_out may only be the first / last schedule entry");
        }
        if (hn->n_in != sn[i].num_inputs || hn->n_out != sn[i].num_outputs)
            return fail(c, FWGPU_ERR_INVALID, "schedule port counts differ from add_node");
        std::string err;
        if (!check_activation(hn->kind, hn->n_in, hn->n_out, err)) return fail(c, FWGPU_ERR_NODE_ACTIVATION_FAILED, err);
        PlanNode pn;
        pn.slot = (uint32_t)(sn[i].node & 0xffffffff);
        pn.kind = hn->kind;
        pn.n_in = (int)hn->n_in;
        pn.n_out = (int)hn->n_out;
        pn.level = 0;
        pn.is_graph_io = pn.slot == c->graph.graph_in_slot ? 1 : (pn.slot == c->graph.graph_out_slot ? 2 : 0);
        pn.in_src_node.assign(pn.n_in, -1);
        pn.in_src_port.assign(pn.n_in, 0);
        for (int p = 0; p < pn.n_in; ++p) {
            if (sn[i].in_should_clear[p]) continue;  // unconnected (InBufferAssignment.should_clear)
            uint32_t b = sn[i].in_buffer_index[p];
            if (b >= num_buffers || last_writer[b].first < 0)
                return fail(c, FWGPU_ERR_INVALID, "schedule input reads a buffer no earlier node wrote");
            pn.in_src_node[p] = last_writer[b].first;
            pn.in_src_port[p] = last_writer[b].second;
        }
        for (int p = 0; p < pn.n_out; ++p) {
            uint32_t b = sn[i].out_buffer_index[p];
            if (b >= num_buffers) return fail(c, FWGPU_ERR_INVALID, "schedule buffer index out of range");
            last_writer[b] = std::make_pair((int)i, p);
        }
        plan.nodes.push_back(pn);
    }
    if (plan.nodes.front().is_graph_io != 1 || plan.nodes.back().is_graph_io != 2)
        return fail(c, FWGPU_ERR_INVALID, "schedule must start with graph_in and end with graph_out");
    finalize_plan(plan);
    RtHold hold(c);  // (as fwgpu_update)
    return install_plan(c, plan);
}

// The introspection calls describe the LATEST BUILT plan (adopted already or waiting for the next process call): the control
// side's own mirror, so they never look at tables the audio side may be swapping.
int fwgpu_plan_kind(fwgpu_ctx* c) {
    if (!c || !c->info.have_plan) return -1;
    if (c->force_generic) return 0;
    return c->info.kind;
}
int fwgpu_plan_fused_voices(fwgpu_ctx* c) {
    if (!c || !c->info.have_plan) return -1;
    return c->force_generic ? 0 : c->info.fused_voices;
}
int fwgpu_plan_num_levels(fwgpu_ctx* c) { return c && c->info.have_plan ? c->info.plan.num_levels : -1; }
int fwgpu_plan_node_level(fwgpu_ctx* c, int64_t node) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (!c->info.have_plan || !c->graph.get(node)) return -1;
    uint32_t slot = (uint32_t)(node & 0xffffffff);
    for (const PlanNode& p : c->info.plan.nodes)
        if (p.slot == slot) return p.level;
    return -1;
}
int fwgpu_plan_node_inputs_clear(fwgpu_ctx* c, int64_t node, int* should_clear, int cap) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (!c->info.have_plan || !c->graph.get(node)) return -1;
    uint32_t slot = (uint32_t)(node & 0xffffffff);
    for (const PlanNode& p : c->info.plan.nodes)
        if (p.slot == slot) {
            for (int i = 0; i < p.n_in && i < cap; ++i) should_clear[i] = p.in_buf[i] == 0 ? 1 : 0;
            return p.n_in;
        }
    return -1;
}
int fwgpu_set_force_generic(fwgpu_ctx* c, int on) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    ControlGate gate(c);
    c->force_generic = on != 0;
    return 0;
}
int fwgpu_plan_handover_stats(fwgpu_ctx* c, uint64_t* adoptions, uint64_t* audio_adoptions, uint64_t* max_adopt_ns) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (adoptions) *adoptions = c->adoptions;
    if (audio_adoptions) *audio_adoptions = c->audio_adoptions;
    if (max_adopt_ns) *max_adopt_ns = c->adopt_ns_max;
    return 0;
}
int fwgpu_plan_pending(fwgpu_ctx* c) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    return c->pending.load(std::memory_order_acquire) != nullptr ? 1 : 0;
}
int fwgpu_lazy_stats(fwgpu_ctx* c, uint64_t* lazy_batches, uint64_t* control_batches) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (lazy_batches) *lazy_batches = c->lazy_calls;
    if (control_batches) *control_batches = c->ctl_calls;
    return 0;
}
int fwgpu_plan_group_stats(fwgpu_ctx* c, uint64_t* grouped_batches) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (grouped_batches) *grouped_batches = c->group_calls;
    return 0;
}
void* fwgpu_hip_stream(fwgpu_ctx* c) { return c ? (void*)c->stream : nullptr; }
int fwgpu_rt_resident_stats(fwgpu_ctx* c, uint64_t* launches, uint64_t* doorbells) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (launches) *launches = c->rtp.launches;
    if (doorbells) *doorbells = c->rtp.doorbells;
    return 0;
}
int fwgpu_rt_path_stats(fwgpu_ctx* c, uint64_t* paths) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (!paths) return fail(c, FWGPU_ERR_INVALID, "null paths");
    for (int i = 0; i < 4; ++i) paths[i] = c->rt_path[i];
    return 0;
}
int fwgpu_plan_chain_stats(fwgpu_ctx* c, uint64_t* steady_workgroups, uint64_t* general_workgroups) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    use_device(c);
    unsigned long long h[2] = {0, 0};
    if (c->d_chain_stats.p) {
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, hipMemcpy(h, c->d_chain_stats.p, sizeof(h), hipMemcpyDeviceToHost));
    }
    if (steady_workgroups) *steady_workgroups = h[0];
    if (general_workgroups) *general_workgroups = h[1];
    return 0;
}
int fwgpu_set_max_batch(fwgpu_ctx* c, uint32_t k) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (k == 0) return fail(c, FWGPU_ERR_INVALID, "max batch must be >= 1");
    c->kmax_req = k;
    c->graph.needs_compile = true;  // K-sized buffers are (re)allocated by the next fwgpu_update
    return 0;
}

static size_t fmt_elem_size(int fmt) { return (fmt == FMT_I_F32 || fmt == FMT_P_F32) ? 4 : 2; }

static int sample_add(fwgpu_ctx* c, int format, uint32_t channels, uint64_t frames, const void* data, bool on_device) {
    use_device(c);
    if (format < 0 || format > FMT_P_F32 || channels == 0) return fail(c, FWGPU_ERR_INVALID, "bad sample format/channels");
    if (frames > (1ull << 40) / channels) return fail(c, FWGPU_ERR_INVALID, "sample too large (frames x channels > 2^40)");
    if (frames && !data) return fail(c, FWGPU_ERR_INVALID, "sample data is null");
    SampleRec r;
    r.alive = true;
    size_t bytes = (size_t)frames * channels * fmt_elem_size(format);
    if (on_device) {
        r.owned = false;
        r.d_data = (void*)data;
    } else {
        r.owned = true;
        HIPC(c, hipMalloc(&r.d_data, bytes + 256));  // slack: a wave's last dwordx4 may overhang the data
        hipError_t e = hipMemset((char*)r.d_data + bytes, 0, 256);
        // (like a plan build's uploads — fwgpu_plan_install.cpp, quiet_window —: in pieces, each when no process call is in flight)
        const bool live = audio_live(c);
        const size_t piece = live ? c->up_piece : (bytes ? bytes : 1);
        for (size_t off = 0; e == hipSuccess && off < bytes; off += piece) {
            if (live) quiet_window(c);
            e = hipMemcpy((char*)r.d_data + off, (const char*)data + off, std::min(piece, bytes - off), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            (void)hipFree(r.d_data);
            return hipfail(c, e, "sample upload");
        }
    }
    r.desc.data = r.d_data;
    r.desc.frames = frames;
    r.desc.channels = (int)channels;
    r.desc.format = format;
    // the data is in HBM; now the table entry — what a process call reads — under the gate: no process call is running, the
    // next one finds the whole entry (and the room for it on the device) in place
    // (a table that has to grow frees its old device copy: hipFree waits for every stream, so the resident realtime kernel is told
    //  to end BEFORE the gate is taken — behind the gate the audio thread could not ring it out, and the free would sit out its
    //  20 ms watchdog with the audio thread parked at its entry: ADVICE r3)
    const bool grows = (c->samples.size() + 1) * sizeof(SampleDesc) > c->d_samples.cap;
    std::unique_ptr<RtHold> hold(grows ? new RtHold(c) : nullptr);
    ControlGate gate(c);
    c->samples.push_back(r);
    c->sample_refs.push_back(0);
    rebuild_sample_table(c);  // copied to the device by the next process / update call; room for it is made here
    if (c->h_sample_tab.size() * sizeof(SampleDesc) > c->d_samples.cap) {
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, c->d_samples.ensure_n("d_samples", c->h_sample_tab.size() * 2 * sizeof(SampleDesc)));
    }
    return (int)c->samples.size() - 1;
}
int fwgpu_sample_create(fwgpu_ctx* c, int format, uint32_t channels, uint64_t frames, const void* data) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    return sample_add(c, format, channels, frames, data, false);
}
int fwgpu_sample_create_device(fwgpu_ctx* c, int format, uint32_t channels, uint64_t frames, const void* device_data) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    return sample_add(c, format, channels, frames, device_data, true);
}
// ---- SPEC streaming sources
int fwgpu_sample_create_stream(fwgpu_ctx* c, int format, uint32_t channels, uint64_t ring_frames) {
    static_assert(FWGPU_STREAM_RING_FRAMES_MAX == SMP_STREAM_RING_MAX && FWGPU_STREAM_RING_MIN_BLOCKS == SMP_STREAM_RING_MIN_BLOCKS, "the header's ring bounds");
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (format < 0 || format > FMT_P_F32 || channels == 0 || channels > 64) return fail(c, FWGPU_ERR_INVALID, "bad sample format/channels");
    if (ring_frames < (uint64_t)SMP_STREAM_RING_MIN_BLOCKS * c->mbf || ring_frames > SMP_STREAM_RING_MAX)
        return fail(c, FWGPU_ERR_INVALID, "fwgpu_sample_create_stream: ring_frames must lie in [4 * max_block_frames, 2^30]");
    use_device(c);
    if (!c->h_stream_pub) {  // the first stream of the ctx: the copy stream, the pinned banks and their events
        RtHold hold(c);  // (pinned allocations wait for the device)
        for (int& sl : c->stream_pub_slot) sl = -1;
        const size_t n = 2 * (size_t)fwgpu_ctx::STREAM_PUB_MAX;
        HIPC(c, hipStreamCreateWithFlags(&c->stream_wr, hipStreamNonBlocking));
        HIPC(c, hipHostMalloc((void**)&c->h_stream_jobs, n * sizeof(BuildJob), hipHostMallocDefault));
        HIPC(c, hipEventCreateWithFlags(&c->ev_stream_pub[0], hipEventDisableTiming));
        HIPC(c, hipEventCreateWithFlags(&c->ev_stream_pub[1], hipEventDisableTiming));
        NodeState* pub = nullptr;
        HIPC(c, hipHostMalloc((void**)&pub, n * sizeof(NodeState), hipHostMallocDefault));
        memset(pub, 0, n * sizeof(NodeState));
        ControlGate gate(c);
        c->h_stream_pub = pub;
    }
    const size_t bytes = (size_t)ring_frames * channels * stream_elem_size(format);
    void* d = nullptr;
    {
        RtHold hold(c);
        HIPC(c, hipMalloc(&d, bytes + 256));  // slack: a wave's last dwordx4 may overhang the data
        const hipError_t e = hipMemset(d, 0, bytes + 256);  // the ring starts zeroed
        if (e != hipSuccess) {
            (void)hipFree(d);
            return hipfail(c, e, "stream ring");
        }
    }
    const int id = sample_add(c, format, channels, ring_frames, d, true);
    if (id < 0) {
        (void)hipFree(d);
        return id;
    }
    c->samples[id].owned = true;  // (the ring is the library's: fwgpu_sample_destroy frees it)
    StreamRec r;
    r.sample = id;
    r.ring = ring_frames;
    c->streams.push_back(r);
    c->samples[id].stream = (int)c->streams.size() - 1;
    return id;
}
static int stream_write_impl(fwgpu_ctx* c, int sample, const void* data, uint64_t frames, bool on_device) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    StreamRec* r = stream_of(c, sample);
    if (!r) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sample_stream_write: not a stream");
    if (r->ended || r->detached) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sample_stream_write: the stream has ended");
    if (frames && !data) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sample_stream_write: data is null");
    use_device(c);
    stream_refresh(c);
    const uint64_t n = std::min<uint64_t>(frames, stream_free(*r));
    if (n == 0) return 0;
    // (the source is laid out as a sample of `frames` frames: a planar channel starts c * frames elements in, whatever is accepted)
    int rc = stream_put(c, *r, data, n, frames, on_device);
    if (rc) return rc;
    rc = stream_tell(c, *r, r->written + n, false, 0);  // a full message ring: `written` does not move, the same call can be repeated
    if (rc) return rc;
    r->written += n;
    return (int)n;
}
int fwgpu_sample_stream_write(fwgpu_ctx* c, int sample, const void* data, uint64_t frames) { return stream_write_impl(c, sample, data, frames, false); }
int fwgpu_sample_stream_write_device(fwgpu_ctx* c, int sample, const void* device_data, uint64_t frames) {
    return stream_write_impl(c, sample, device_data, frames, true);
}
int fwgpu_sample_stream_end(fwgpu_ctx* c, int sample) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    StreamRec* r = stream_of(c, sample);
    if (!r) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sample_stream_end: not a stream");
    if (r->ended && !r->detached && r->node >= 0 && !r->end_told) {
        // ended before it was bound, and the binding found no room for the message that carries E: the same call delivers it
        const int rc = stream_tell(c, *r, r->written, true, r->end_at);
        if (rc == 0) r->end_told = true;
        return rc;
    }
    if (r->ended || r->detached) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sample_stream_end: the stream has ended");
    use_device(c);
    stream_refresh(c);
    if (stream_free(*r) < c->mbf) return fail(c, FWGPU_ERR_QUEUE_FULL, "fwgpu_sample_stream_end: no room yet for the padding behind the data");
    int rc = stream_put(c, *r, nullptr, c->mbf, c->mbf, false);
    if (rc) return rc;
    rc = stream_tell(c, *r, r->written + c->mbf, true, r->written);
    if (rc) return rc;
    r->end_at = r->written;
    r->written += c->mbf;
    r->ended = true;
    r->end_told = r->node >= 0 && !r->detached;  // (not bound yet: the end travels behind the binding)
    return 0;
}
int fwgpu_sample_stream_status(fwgpu_ctx* c, int sample, uint64_t* written, uint64_t* consumed, uint64_t* starved_blocks, int* finished) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    StreamRec* r = stream_of(c, sample);
    if (!r) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sample_stream_status: not a stream");
    use_device(c);
    stream_refresh(c);
    if (written) *written = r->ended ? r->end_at : r->written;
    if (consumed) *consumed = r->consumed;
    if (starved_blocks) *starved_blocks = r->starved;
    if (finished) *finished = r->finished ? 1 : 0;
    return 0;
}
int fwgpu_sample_destroy(fwgpu_ctx* c, int sample) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (sample < 0 || sample >= (int)c->samples.size() || !c->samples[sample].alive)
        return fail(c, FWGPU_ERR_INVALID, "unknown sample id");
    // FIR / resampler nodes name their sample at construction and keep it for life: refuse while one exists.  Samplers
    // pick samples by message, which the host does not track: see the contract in fwgpu.h.
    for (const HostNode& n : c->graph.nodes)
        if ((n.alive && n.kind == K_RESAMPLER && n.init.sample == sample) || fir_uses_sample(n, sample))
            return fail(c, FWGPU_ERR_INVALID, "sample is in use by a FIR / resampler node");
    use_device(c);
    RtHold hold(c);       // the resident realtime kernel ends now, and none is launched until the data is gone
    ControlGate gate(c);  // no process call runs while the entry is emptied and the data freed
    (void)rt_persist_stop(c);  // ... and no resident realtime kernel: between two callbacks it may be fetching the frames a voice reads next
    (void)hipStreamSynchronize(c->stream);
    if (c->ctl_stream) (void)hipStreamSynchronize(c->ctl_stream);
    SampleRec& r = c->samples[sample];
    if (r.stream >= 0) {  // (the gate is held: the table entry is cleared by hand, stream_pub_drop would take it again)
        StreamRec& sr = c->streams[r.stream];
        if (sr.pub >= 0) {
            c->stream_pub_slot[sr.pub] = -1;
            c->stream_pub_n--;
            sr.pub = -1;
        }
        sr.detached = sr.finished = true;
        // (the sampler that held it holds a stream no longer: seek and loop messages are accepted on it again)
        if (HostNode* hn = sr.node >= 0 ? c->graph.get(sr.node) : nullptr)
            if (hn->stream == r.stream) hn->stream = -1;
        if (c->stream_wr) (void)hipStreamSynchronize(c->stream_wr);
    }
    if (r.owned && r.d_data) (void)hipFree(r.d_data);
    r.alive = false;
    r.d_data = nullptr;
    r.desc.data = nullptr;
    r.desc.frames = 0;
    rebuild_sample_table(c);
    return 0;
}

int fwgpu_poll_returned_samples(fwgpu_ctx* c, int64_t* nodes, int* samples, int cap) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (cap < 0 || (cap > 0 && (!nodes || !samples))) return fail(c, FWGPU_ERR_INVALID, "null output arrays");
    use_device(c);
    collect_returns(c);
    int n = 0;
    for (; n < cap && (size_t)n < c->ret_ready.size(); ++n) {
        nodes[n] = c->ret_ready[n].node;
        samples[n] = c->ret_ready[n].sample;
    }
    c->ret_ready.erase(c->ret_ready.begin(), c->ret_ready.begin() + n);
    return n;
}
int fwgpu_sample_retired(fwgpu_ctx* c, int sample) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (sample < 0 || sample >= (int)c->samples.size()) return fail(c, FWGPU_ERR_INVALID, "unknown sample id");
    use_device(c);
    collect_returns(c);
    for (const HostNode& n : c->graph.nodes)
        if ((n.alive && n.kind == K_RESAMPLER && n.init.sample == sample) || fir_uses_sample(n, sample)) return 0;
    return c->sample_refs[sample] == 0 ? 1 : 0;
}
int fwgpu_ext_pool_floats(fwgpu_ctx* c, uint64_t* in_use, uint64_t* capacity) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (in_use) *in_use = (uint64_t)c->ext_used;
    if (capacity) *capacity = (uint64_t)c->ext_cap;
    return 0;
}

// The automation curve of fwgpu_crossfade_to, fwgpu_fir_morph and fwgpu_gain_ride (`who`): the shape, x in 0..1, y in -1..2.  0: the
// curve is good; else the refusal, reported in the caller's name
static int refuse_bad_curve(fwgpu_ctx* c, const char* who, int shape, float x1, float y1, float x2, float y2) {
    if (shape != XF_SHAPE_LINEAR && shape != XF_SHAPE_BEZIER) return fail(c, FWGPU_ERR_INVALID, who, "shape must be 0 (linear) or 1 (Bezier)");
    if (!(x1 >= 0.0f && x1 <= 1.0f && x2 >= 0.0f && x2 <= 1.0f)) return fail(c, FWGPU_ERR_INVALID, who, "x1 and x2 must be in 0..1");
    if (!(y1 >= -1.0f && y1 <= 2.0f && y2 >= -1.0f && y2 <= 2.0f)) return fail(c, FWGPU_ERR_INVALID, who, "y1 and y2 must be in -1..2");
    return 0;
}
// SPEC crossfader: one CMD_XF_TO; position and x in 0..1, y in -1..2, at most 2^24 frames
int fwgpu_crossfade_to(fwgpu_ctx* c, int64_t node, float position, uint32_t frames, int shape, float x1, float y1, float x2, float y2,
                       uint32_t at_block) {
    static_assert(FWGPU_CROSSFADE_FRAMES_MAX == XF_FRAMES_MAX && FWGPU_CROSSFADE_CH_MAX == XF_CH_MAX, "the header's crossfader caps");
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (n->kind != K_CROSSFADE) return fail(c, FWGPU_ERR_INVALID, "fwgpu_crossfade_to: the node is not a CrossfadeNode");
    if (!(position >= 0.0f && position <= 1.0f)) return fail(c, FWGPU_ERR_INVALID, "fwgpu_crossfade_to: position must be in 0..1");
    if (frames > FWGPU_CROSSFADE_FRAMES_MAX) return fail(c, FWGPU_ERR_INVALID, "fwgpu_crossfade_to: at most 2^24 frames");
    if (int rc = refuse_bad_curve(c, "fwgpu_crossfade_to", shape, x1, y1, x2, y2)) return rc;
    return push_cmd(c, node, K_CROSSFADE, make_xf_to(at_block, position, frames, shape, x1, y1, x2, y2), false);
}
// SPEC FIR morph: one CMD_XF_TO for a morph-capable FirReverbNode, with fwgpu_crossfade_to's refusals.  The host keeps
// the last morph's target and end (HostNode::fir_target, fir_target_end) — what fwgpu_fir_set_ir asks before it exchanges a slot
int fwgpu_fir_morph(fwgpu_ctx* c, int64_t node, float position, uint32_t frames, int shape, float x1, float y1, float x2, float y2,
                    uint32_t at_block) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (n->kind != K_FIR || !n->fir_morph) return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_morph: the node is not a morph-capable FirReverbNode");
    if (!(position >= 0.0f && position <= 1.0f)) return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_morph: position must be in 0..1");
    if (frames > XF_FRAMES_MAX) return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_morph: at most 2^24 frames");
    if (int bad = refuse_bad_curve(c, "fwgpu_fir_morph", shape, x1, y1, x2, y2)) return bad;
    Cmd m = make_xf_to(at_block, position, frames, shape, x1, y1, x2, y2);
    int rc;
    // held: the message waits in early_msgs — for the plan that activates the node, or for the one that holds a fwgpu_fir_set_ir — and
    // starts only behind the update that releases it; process calls on the old plan may render any number of frames before that, so
    // the book is written at the release (fwgpu_plan_install.cpp publish), and until then both slots count as audible
    const bool held = !n->activated || n->fir_hold;
    if (n->activated && n->fir_hold) {  // a fwgpu_fir_set_ir waits for its plan: held like a message for a node that is not activated yet
        m.state = (int)(node & 0xffffffff);
        if (c->early_msgs.size() >= fwgpu_ctx::RING_CAP) return fail(c, FWGPU_ERR_QUEUE_FULL, "too many held messages");
        c->early_msgs.push_back(m);
        rc = 0;
    } else {
        rc = push_cmd(c, node, K_FIR, m, false);
    }
    if (rc == 0) {
        if (held) n->fir_held++;
        else fir_note_morph(*n, position, c->frames_ctl.load(std::memory_order_acquire) + (uint64_t)at_block * c->mbf, frames);
    }
    return rc;
}
// SPEC FIR morph: exchange the impulse response of a slot nobody hears — a graph edit, adopted with the plan the next update builds
int fwgpu_fir_set_ir(fwgpu_ctx* c, int64_t node, int slot, int sample) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (n->kind != K_FIR || !n->fir_morph) return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_set_ir: the node is not a morph-capable FirReverbNode");
    if (slot != 0 && slot != 1) return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_set_ir: slot must be 0 (A) or 1 (B)");
    if (sample == -1 && slot == 0) return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_set_ir: slot A cannot be emptied (its rows append the history)");
    if (sample != -1) {
        if (sample < 0 || sample >= (int)c->samples.size() || !c->samples[sample].alive || c->samples[sample].desc.frames == 0)
            return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_set_ir: sample must be -1 or the id of a non-empty impulse-response sample");
        if (c->samples[sample].stream >= 0) return fail(c, FWGPU_ERR_INVALID, "a stream cannot be an impulse response or a resampler's source");
        const uint64_t cap = n->activated ? n->init.loop_start : (n->fir_max_taps ? n->fir_max_taps : (1u << 24));
        if (c->samples[sample].desc.frames > cap) return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_set_ir: the sample is longer than the node's tap capacity");
    }
    // inaudible: no morph waits to be released, the last morph queued (or the creation position) targets exactly the other slot's end,
    // and its last frame lies behind the frames of every process call started so far (the edit is adopted by a later call's plan)
    const float other_end = slot == 0 ? 1.0f : 0.0f;
    if (n->fir_held || n->fir_target != other_end || n->fir_target_end > c->frames_ctl.load(std::memory_order_acquire))
        return fail(c, FWGPU_ERR_INVALID, "fwgpu_fir_set_ir: the slot is audible (morph to the other slot's end and render the fade first)");
    const int old = n->fir_ir[slot];
    if (old == sample) return 0;
    n->fir_ir[slot] = sample;
    if (!n->activated && slot == 0) n->init.sample = sample;
    if (n->activated) n->fir_hold = true;
    c->graph.needs_compile = true;
    if (old != n->fir_ir[slot ^ 1]) fir_ir_release(c, old);
    return 0;
}
int fwgpu_fir_morph_stats(fwgpu_ctx* c, uint64_t* tiles_run, uint64_t* tiles_skipped) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    unsigned long long h[2] = {0ull, 0ull};
    if (c->d_fir_stats.p) {
        use_device(c);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(h, c->d_fir_stats.p, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, FWGPU_ERR_DEVICE, "fwgpu_fir_morph_stats: reading the counters failed");
    }
    if (tiles_run) *tiles_run = (uint64_t)h[0];
    if (tiles_skipped) *tiles_skipped = (uint64_t)h[1];
    return 0;
}
// SPEC resampler ratio glide: one CMD_RS_GLIDE to param 1's resampler_step of the ratio; frames == 0 is param 1's
// message, a step.  Any ratio but a NaN, at most 2^24 frames
int fwgpu_resampler_glide(fwgpu_ctx* c, int64_t node, float ratio, uint32_t frames, uint32_t at_block) {
    static_assert(FWGPU_RESAMPLER_GLIDE_FRAMES_MAX == RS_GLIDE_FRAMES_MAX, "the header's glide cap");
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (n->kind != K_RESAMPLER) return fail(c, FWGPU_ERR_INVALID, "fwgpu_resampler_glide: the node is not a resampling source");
    if (ratio != ratio) return fail(c, FWGPU_ERR_INVALID, "fwgpu_resampler_glide: ratio is NaN");
    if (frames > FWGPU_RESAMPLER_GLIDE_FRAMES_MAX) return fail(c, FWGPU_ERR_INVALID, "fwgpu_resampler_glide: at most 2^24 frames");
    return push_cmd(c, node, -1, make_rs_step(at_block, resampler_step(ratio), frames), false);
}
int fwgpu_node_set_param(fwgpu_ctx* c, int64_t node, int param, float value, uint32_t at_block) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    const auto push = [&](const Cmd& m) { return push_cmd(c, node, -1, m, false); };
    switch (n->kind) {
        case K_VOLUME:
        case K_SAMPLER:  // volume.rs:28-34, sampler.rs:171-177
            if (param != 0) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            return push(make_set(CMD_SET_P0, at_block, percent_volume_to_raw_gain(value)));
        case K_BEEP:  // beep_test.rs:30-32
            if (param != 0) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            return push(make_set_enabled(at_block, value != 0.0f));
        case K_PAN: {
            if (param != 0) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            float gl, gr;
            pan_to_gains(value, &gl, &gr);
            const int rc = push(make_set(CMD_SET_P0, at_block, gl));
            return rc ? rc : push(make_set(CMD_SET_P1, at_block, gr));
        }
        case K_WIDTH:
            if (param != 0) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            return push(make_set(CMD_SET_P0, at_block, fmaxf(value, 0.0f)));
        case K_BIQUAD: {  // param 1 = cutoff_hz, 2 = Q: recompute the coefficients on the control side
            if (param != 1 && param != 2) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            if (param == 1) n->init.p0 = value;
            else n->init.p1 = value;
            float co[5];
            biquad_coefs(n->init.enabled, n->init.p0, n->init.p1, c->sample_rate, co);
            return push(make_bq_coefs(at_block, co, 0u));
        }
        case K_DELAY: {  // param 1 = feedback, 2 = mix (the delay time is fixed at construction)
            if (param == 1) return push(make_set(CMD_SET_P0, at_block, fminf(fmaxf(value, 0.0f), 0.999f)));
            if (param != 2) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            const float mix = fminf(fmaxf(value, 0.0f), 1.0f);
            const int rc = push(make_set(CMD_SET_P1, at_block, mix));
            return rc ? rc : push(make_set(CMD_SET_GAIN, at_block, 1.0f - mix));
        }
        case K_RESAMPLER:  // 1 = ratio (source frames per output frame), 3 = playing, 4 = seek to a source frame
            if (param == 1) return push(make_rs_step(at_block, resampler_step(value), 0u));
            if (param == 3) return push(make_smp_transport(value != 0.0f ? CMD_SMP_PLAY : CMD_SMP_PAUSE, at_block));
            if (param != 4) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            return push(make_rs_seek(at_block, (uint64_t)fmaxf(value, 0.0f)));
        case K_SPATIAL: {  // 0 / 1 / 2 = x / y / z of the source relative to the listener
            if (param < 0 || param > 2) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            if (param == 0) n->init.phasor = value;
            else if (param == 1) n->init.phasor_inc = value;
            else n->init.gain = value;
            float gl, gr;
            int dl, dr;
            spatial_params(n->init.phasor, n->init.phasor_inc, n->init.gain, c->sample_rate, &gl, &gr, &dl, &dr);
            int rc = push(make_set(CMD_SET_P0, at_block, gl));
            if (rc) return rc;
            if ((rc = push(make_set(CMD_SET_P1, at_block, gr)))) return rc;
            return push(make_sp_itd(at_block, gr, dl, dr));
        }
        case K_CROSSFADE:  // param 0 = position: a jump (fwgpu_crossfade_to with frames 0)
            if (param != 0) return fail(c, FWGPU_ERR_INVALID, "unknown param");
            return fwgpu_crossfade_to(c, node, value, 0, XF_SHAPE_LINEAR, 0.0f, 0.0f, 1.0f, 1.0f, at_block);
        case K_LIMITER:  // ceiling and hold are fixed at construction (a moving ceiling would need a smoother: out of scope)
            return fail(c, FWGPU_ERR_INVALID, "LimiterNode has no runtime params: ceiling and hold_frames are set at add_node");
        case K_DUCKER:  // threshold, depth and the three times are fixed at construction (moving ones: out of scope)
            return fail(c, FWGPU_ERR_INVALID, "DuckerNode has no runtime params: threshold, depth, attack, release and hold are set at add_node");
        case K_COMPRESSOR:  // the curve, the times and the makeup are fixed at construction (moving ones: out of scope)
            static_assert(FWGPU_COMPRESSOR == K_COMPRESSOR && FWGPU_COMPRESSOR_WIN_MAX == COMP_WIN_MAX && FWGPU_COMPRESSOR_HOLD_MAX == COMP_HOLD_MAX &&
                              FWGPU_COMPRESSOR_CH_MAX == COMP_CH_MAX, "the header's compressor kind and caps");
            return fail(c, FWGPU_ERR_INVALID,
                        "CompressorNode has no runtime params: threshold, ratio, knee, attack, release, hold and makeup are set at add_node");
        case K_DELAY_COMP:  // the delay is fixed at construction (a moving one would be an effect: FWGPU_DELAY)
            return fail(c, FWGPU_ERR_INVALID, "DelayCompNode has no runtime params: frames is set at add_node");
        default:
            return fail(c, FWGPU_ERR_INVALID, "node kind has no runtime params");
    }
}
// SPEC biquad coefficient sweep: one CMD_BQ_SWEEP to the coefficients param 1 / 2 would set; frames == 0 is their
// message, a step.  Any cutoff and Q but a NaN, at most 2^24 frames
int fwgpu_biquad_sweep(fwgpu_ctx* c, int64_t node, float cutoff_hz, float q, uint32_t frames, uint32_t at_block) {
    static_assert(FWGPU_BIQUAD_SWEEP_FRAMES_MAX == BQ_SWEEP_FRAMES_MAX, "the header's sweep cap");
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (n->kind != K_BIQUAD) return fail(c, FWGPU_ERR_INVALID, "fwgpu_biquad_sweep: the node is not a BiquadNode");
    if (cutoff_hz != cutoff_hz || q != q) return fail(c, FWGPU_ERR_INVALID, "fwgpu_biquad_sweep: cutoff_hz or q is NaN");
    if (frames > FWGPU_BIQUAD_SWEEP_FRAMES_MAX) return fail(c, FWGPU_ERR_INVALID, "fwgpu_biquad_sweep: at most 2^24 frames");
    n->init.p0 = cutoff_hz;  // (a later set_param of Q alone starts from these)
    n->init.p1 = q;
    float co[5];
    biquad_coefs(n->init.enabled, cutoff_hz, q, c->sample_rate, co);
    return push_cmd(c, node, -1, make_bq_coefs(at_block, co, frames), false);
}
// SPEC spatialiser move: one CMD_SP_MOVE to what params 0..2 would set for (x, y, z); frames == 0 is their three
// position messages (CMD_SET_P0, CMD_SET_P1, CMD_SP_ITD), a step.  Any coordinates but a NaN, at most 2^24 frames
int fwgpu_spatial_move(fwgpu_ctx* c, int64_t node, float x, float y, float z, uint32_t frames, uint32_t at_block) {
    static_assert(FWGPU_SPATIAL_MOVE_FRAMES_MAX == SP_MOVE_FRAMES_MAX, "the header's move cap");
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (n->kind != K_SPATIAL) return fail(c, FWGPU_ERR_INVALID, "fwgpu_spatial_move: the node is not a SpatialNode");
    if (x != x || y != y || z != z) return fail(c, FWGPU_ERR_INVALID, "fwgpu_spatial_move: a coordinate is NaN");
    if (frames > FWGPU_SPATIAL_MOVE_FRAMES_MAX) return fail(c, FWGPU_ERR_INVALID, "fwgpu_spatial_move: at most 2^24 frames");
    float gl, gr;
    int dl, dr;
    spatial_params(x, y, z, c->sample_rate, &gl, &gr, &dl, &dr);
    int rc;
    if (frames != 0u) {
        rc = push_cmd(c, node, -1, make_sp_move(at_block, gl, gr, dl, dr, frames), false);
    } else {  // the three messages the LAST of three set_param calls for that position queues (its first two calls' six are overwritten by them)
        rc = push_cmd(c, node, -1, make_set(CMD_SET_P0, at_block, gl), false);
        if (!rc) rc = push_cmd(c, node, -1, make_set(CMD_SET_P1, at_block, gr), false);
        if (!rc) rc = push_cmd(c, node, -1, make_sp_itd(at_block, gr, dl, dr), false);
    }
    if (rc) return rc;  // (a refused call leaves the node's recorded position alone)
    n = c->graph.get(node);
    if (n) {  // a later set_param of one coordinate starts from these
        n->init.phasor = x;
        n->init.phasor_inc = y;
        n->init.gain = z;
    }
    return 0;
}
// SPEC gain ride: one CMD_GAIN_RIDE to the gain or gains param 0 would set for `value`; frames == 0 is a step with no
// glide.  The curve is the crossfader's and is validated as fwgpu_crossfade_to validates it; at most 2^24 frames
int fwgpu_gain_ride(fwgpu_ctx* c, int64_t node, float value, uint32_t frames, int shape, float x1, float y1, float x2, float y2, uint32_t at_block) {
    static_assert(FWGPU_GAIN_RIDE_FRAMES_MAX == GAIN_RIDE_FRAMES_MAX, "the header's ride cap");
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (n->kind != K_VOLUME && n->kind != K_PAN) return fail(c, FWGPU_ERR_INVALID, "fwgpu_gain_ride: the node is not a VolumeNode or a StereoPanNode");
    if (!(value - value == 0.0f)) return fail(c, FWGPU_ERR_INVALID, "fwgpu_gain_ride: value is NaN or infinite");
    if (frames > FWGPU_GAIN_RIDE_FRAMES_MAX) return fail(c, FWGPU_ERR_INVALID, "fwgpu_gain_ride: at most 2^24 frames");
    if (int rc = refuse_bad_curve(c, "fwgpu_gain_ride", shape, x1, y1, x2, y2)) return rc;
    float g0, g1 = 0.0f;  // (a volume has one gain: its second target stays where make_state leaves p1)
    if (n->kind == K_VOLUME) g0 = percent_volume_to_raw_gain(value);
    else pan_to_gains(value, &g0, &g1);
    return push_cmd(c, node, -1, make_gain_ride(at_block, g0, g1, frames, shape, x1, y1, x2, y2), false);
}
int fwgpu_node_set_params(fwgpu_ctx* c, uint32_t n, const int64_t* nodes, const int* params, const float* values, const uint32_t* at_blocks) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (n && (!nodes || !params || !values || !at_blocks)) return fail(c, FWGPU_ERR_INVALID, "null message list");
    for (uint32_t i = 0; i < n; ++i) {
        const int rc = fwgpu_node_set_param(c, nodes[i], params[i], values[i], at_blocks[i]);
        if (rc < 0) return rc;
    }
    return 0;
}
int fwgpu_sampler_set_sample(fwgpu_ctx* c, int64_t node, int sample, int stop_playback, uint32_t at_block) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (sample < 0 || sample >= (int)c->samples.size() || !c->samples[sample].alive)
        return fail(c, FWGPU_ERR_INVALID, "unknown sample id");
    // SPEC streaming source: a stream is bound once, to one sampler; the message carries R and the current W
    StreamRec* sr = stream_of(c, sample);
    HostNode* hn = c->graph.get(node);
    int pub = -1;
    if (sr) {
        if (!hn || hn->kind != K_SAMPLER) return fail(c, FWGPU_ERR_INVALID, "node kind does not accept this message");
        if (sr->node >= 0 || sr->detached) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_set_sample: a stream is bound once, to one sampler");
        for (int i = 0; i < fwgpu_ctx::STREAM_PUB_MAX && pub < 0; ++i)
            if (c->stream_pub_slot[i] < 0) pub = i;
        if (pub < 0) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_set_sample: too many samplers hold a stream (64)");
    }
    int rc = push_cmd(c, node, K_SAMPLER, make_smp_set_sample(at_block, sample, stop_playback != 0, sr ? sr->ring : 0, sr ? sr->written : 0), true);
    if (rc) return rc;
    c->sample_refs[sample]++;  // the message carries the reference (an Arc clone in the reference: sampler.rs:67-79)
    if (hn && hn->stream >= 0 && hn->stream < (int)c->streams.size()) stream_detach(c, c->streams[hn->stream]);  // the stream it held is finished
    if (hn) hn->stream = sr ? (int)(sr - c->streams.data()) : -1;
    if (sr) {
        sr->node = node;
        {
            ControlGate gate(c);
            c->stream_pub_slot[pub] = (int)(node & 0xffffffff);
            c->stream_pub_n++;
        }
        sr->pub = pub;
        if (sr->ended) {  // (ended before it was bound: the end travels behind the binding)
            rc = stream_tell(c, *sr, sr->written, true, sr->end_at);
            // no room for it (FWGPU_ERR_QUEUE_FULL): the binding stands, and fwgpu_sample_stream_end, called again, delivers the end
            if (rc) return rc;
            sr->end_told = true;
        }
    }
    return 0;
}
int fwgpu_sampler_play(fwgpu_ctx* c, int64_t node, uint32_t b) { return c ? push_cmd(c, node, K_SAMPLER, make_smp_transport(CMD_SMP_PLAY, b), true) : FWGPU_ERR_INVALID; }
int fwgpu_sampler_pause(fwgpu_ctx* c, int64_t node, uint32_t b) { return c ? push_cmd(c, node, K_SAMPLER, make_smp_transport(CMD_SMP_PAUSE, b), true) : FWGPU_ERR_INVALID; }
int fwgpu_sampler_stop(fwgpu_ctx* c, int64_t node, uint32_t b) { return c ? push_cmd(c, node, K_SAMPLER, make_smp_transport(CMD_SMP_STOP, b), true) : FWGPU_ERR_INVALID; }
// SPEC sampler gain envelope: one CMD_SMP_FADE; a target in 0..1 (-0.0 counts as +0.0), at most 2^24 frames, a `then`
// only behind a fade that has frames
int fwgpu_sampler_fade(fwgpu_ctx* c, int64_t node, float target, uint32_t frames, int then, uint32_t at_block) {
    static_assert(FWGPU_SAMPLER_FADE_FRAMES_MAX == SMP_FADE_FRAMES_MAX, "the header's fade cap");
    static_assert(FWGPU_FADE_NONE == SMP_FADE_NONE && FWGPU_FADE_PAUSE == SMP_FADE_PAUSE && FWGPU_FADE_STOP == SMP_FADE_STOP, "the header's fade ends");
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HostNode* n = c->graph.get(node);
    if (!n) return fail(c, FWGPU_ERR_INVALID, "unknown node id");
    if (n->kind != K_SAMPLER) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_fade: the node is not a SamplerNode");
    if (!(target >= 0.0f && target <= 1.0f)) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_fade: target must be in 0..1");
    if (frames > FWGPU_SAMPLER_FADE_FRAMES_MAX) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_fade: at most 2^24 frames");
    if (then < FWGPU_FADE_NONE || then > FWGPU_FADE_STOP) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_fade: then must be 0 (none), 1 (pause) or 2 (stop)");
    if (frames == 0 && then != FWGPU_FADE_NONE)
        return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_fade: a step (frames 0) has no end to pause or stop at: use fwgpu_sampler_pause / _stop");
    return push_cmd(c, node, K_SAMPLER, make_smp_fade(at_block, target == 0.0f ? 0.0f : target, frames, then), true);  // (-0.0 counts as +0.0)
}
int fwgpu_sampler_set_playhead_secs(fwgpu_ctx* c, int64_t node, double secs, uint32_t at_block) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (HostNode* hn = c->graph.get(node))
        if (hn->stream >= 0) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_set_playhead_secs: the sampler holds a stream: there is no position to seek to");
    return push_cmd(c, node, K_SAMPLER, make_smp_set_playhead(at_block, secs), true);
}
int fwgpu_sampler_set_loop_range(fwgpu_ctx* c, int64_t node, int mode, double start, double end, uint32_t at_block) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (mode < 0 || mode > 2) return fail(c, FWGPU_ERR_INVALID, "loop mode must be 0, 1 or 2");
    if (HostNode* hn = c->graph.get(node))
        if (hn->stream >= 0) return fail(c, FWGPU_ERR_INVALID, "fwgpu_sampler_set_loop_range: the sampler holds a stream: there is no range to loop");
    return push_cmd(c, node, K_SAMPLER, make_smp_set_loop(at_block, mode, start, end), true);
}

static int process_interleaved_impl(fwgpu_ctx* c, const float* input, float* output, uint32_t n_in_ch, uint32_t n_out_ch,
                                    uint64_t frames, size_t out_bytes) {
    const float* d_in = nullptr;
    const size_t in_bytes_rt = (n_in_ch > 0 && input) ? (size_t)frames * n_in_ch * sizeof(float) : 0;
    if (c->h_rt_out && out_bytes <= RT_IO_BYTES && in_bytes_rt <= RT_IO_BYTES) {
        // realtime-sized call: graph inputs are read from, and the interleaved output written to, pinned host blocks
        // mapped into the device — the only wait is the stream sync (SURVEY 8(b) "realtime rules")
        if (in_bytes_rt) {
            memcpy(c->h_rt_in, input, in_bytes_rt);
            d_in = c->d_rt_in;
        }
        const bool spin = c->h_rt_flag != nullptr && !c->rt_use_graph;
        c->rt_signal_seq = spin ? ++c->rt_seq : 0;
        c->rt_signalled = false;
        int rc = run_blocks(c, frames, d_in, (int)n_in_ch, c->d_rt_out, (int)n_out_ch, true);
        c->rt_signal_seq = 0;
        if (rc) return rc;
        bool done = false;
        if (spin && c->rt_signalled) {
            // poll the completion flag (plain loads of pinned memory: no driver call, no sleep); a device that has not
            // answered after ~20 ms of spinning has a problem the stream sync below will name
            const unsigned long long want = c->rt_seq;
            volatile unsigned long long* flag = c->h_rt_flag;
            for (int attempt = 0; attempt < 2 && !done; ++attempt) {
                bool retry = false;
                // (bounded by the CLOCK, looked at every 1024 polls: an iteration count of `pause`s was ~1 s, not 20 ms — ADVICE r2)
                const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
                for (unsigned spins = 1;; ++spins) {
                    if (*flag == want) {
                        done = true;
                        break;
                    }
                    // the resident kernel's watchdog fired between two callbacks and the doorbell came too late for it: it says so
                    // (alive = 0, stored after its last completion flag) — this block has not been rendered and will not be
                    if (c->rtp.launched && (spins & 63u) == 0 && !*(volatile unsigned long long*)&c->h_rt_mb->alive) {
                        std::atomic_thread_fence(std::memory_order_acquire);
                        if (*flag != want) {
                            retry = true;
                            break;
                        }
                    }
#if defined(__x86_64__) || defined(__i386__)
                    __builtin_ia32_pause();
#endif
                    if ((spins & 1023u) == 0 && std::chrono::steady_clock::now() > give_up) break;
                }
                if (!retry) break;
                rc = rt_block_relaunch(c, c->d_rt_out, want);  // (rare: a pause of the watchdog's length) the block as an ordinary launch
                if (rc) return rc;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
        }
        if (!done) {
            if (c->rtp.launched) HIPC(c, hipStreamSynchronize(c->rt_stream));
            HIPC(c, hipStreamSynchronize(c->stream));
            // the streams are empty — which says the block was rendered only if its completion flag says so too: a resident kernel that
            // waited for another number has ended on its watchdog WITHOUT rendering this one.  One ordinary launch of the
            // block, then the flag must be there; stale audio is never copied out as if it were this block's.
            if (spin && c->rt_signalled && *(volatile unsigned long long*)c->h_rt_flag != c->rt_seq) {
                rc = rt_block_relaunch(c, c->d_rt_out, c->rt_seq);
                if (rc) return rc;
                HIPC(c, hipStreamSynchronize(c->stream));
                if (*(volatile unsigned long long*)c->h_rt_flag != c->rt_seq)
                    return fail(c, FWGPU_ERR_DEVICE, "realtime block was not rendered (completion flag missing after a stream sync)");
            }
        }
        c->ret_done_ticket.store(c->ret_ticket, std::memory_order_release);  // everything this call handed back is final
        if (out_bytes) memcpy(output, c->h_rt_out, out_bytes);
        return 0;
    }
    if (n_in_ch > 0 && input) {
        size_t in_bytes = (size_t)frames * n_in_ch * sizeof(float);
        if (in_bytes > c->d_in_stage.cap) {  // (first call of this size only)
            HIPC(c, hipStreamSynchronize(c->stream));
            HIPC(c, c->d_in_stage.ensure_n("d_in_stage", in_bytes));
        }
        HIPC(c, hipMemcpyAsync(c->d_in_stage.p, input, in_bytes, hipMemcpyHostToDevice, c->stream));
        d_in = c->d_in_stage.as<float>();
    }
    if (out_bytes > c->d_out_stage.cap) {
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, c->d_out_stage.ensure_n("d_out_stage", out_bytes));
    }
    int rc = run_blocks(c, frames, d_in, (int)n_in_ch, c->d_out_stage.as<float>(), (int)n_out_ch);
    if (rc) return rc;
    if (out_bytes) HIPC(c, hipMemcpyAsync(output, c->d_out_stage.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->ret_done_ticket.store(c->ret_ticket, std::memory_order_release);
    return 0;
}

int fwgpu_process_interleaved(fwgpu_ctx* c, const float* input, float* output, uint32_t n_in_ch, uint32_t n_out_ch,
                              uint64_t frames, double stream_time_secs, uint32_t stream_status) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    if (n_in_ch > 64 || n_out_ch > 64) return fail(c, FWGPU_ERR_INVALID, "at most 64 stream channels per side (processor.rs:43-44)");
    if (frames > (1ull << 32)) return fail(c, FWGPU_ERR_INVALID, "more than 2^32 frames in one call");
    size_t out_bytes = (size_t)frames * n_out_ch * sizeof(float);
    if (out_bytes && !output) return fail(c, FWGPU_ERR_INVALID, "output is null");
    // ProcInfo::stream_time_secs / stream_status of this call (core/node.rs:111-118): no built-in node reads them; a
    // custom node mixed in through fwgpu_node_process gets them from fwgpu_proc_info
    AudioGate gate(c);  // (picks up a plan the control thread published since the last call: processor.rs:167-206)
    c->proc_stream_time = stream_time_secs;
    c->proc_stream_status = stream_status;
    if (stream_status & 2u) c->n_underflows++;
    if (stream_status & 1u) c->n_overflows++;
    if (!c->have_plan || frames == 0) {  // processor.rs:86-89 (Q19)
        if (out_bytes) memset(output, 0, out_bytes);
        return 0;
    }
    const int rc = process_interleaved_impl(c, input, output, n_in_ch, n_out_ch, frames, out_bytes);
    // "all output buffers MUST be filled" (core/node.rs:41-42): whatever failed — a launch, the wait for the stream, the
    // copy back — the caller's buffer never keeps what it held before the call
    if (rc != 0 && out_bytes) memset(output, 0, out_bytes);
    return rc;
}
// ---- the call split in two (include/fwgpu.h): render n + 1 while call n's output crosses PCIe into the caller's buffer
// (Round 5, measured on config 2, 1.5 MiB per call: staging in hipHostMalloc memory + memcpy in `end`: 0.67 ms per step against 0.345 for
//  the synchronous call — the host's memcpy out of that memory; the copy issued by `end` straight into the caller's pageable buffer:
//  0.318 against 0.312 — a blit kernel that queues behind the next ticket's kernels, no overlap.  Hence registered ordinary memory.)
int64_t fwgpu_process_interleaved_begin(fwgpu_ctx* c, const float* input, uint32_t n_in_ch, uint32_t n_out_ch, uint64_t frames,
                                        double stream_time_secs, uint32_t stream_status) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    if (n_in_ch > 64 || n_out_ch > 64) return fail(c, FWGPU_ERR_INVALID, "at most 64 stream channels per side (processor.rs:43-44)");
    if (frames > (1ull << 32)) return fail(c, FWGPU_ERR_INVALID, "more than 2^32 frames in one call");
    fwgpu_ctx::AsyncOut& a = c->ao;
    const int slot = (int)(a.next & 1);
    if (a.busy[slot]) return fail(c, FWGPU_ERR_INVALID, "two calls in flight already: end the older ticket first");
    const size_t out_bytes = (size_t)frames * n_out_ch * sizeof(float);
    AudioGate gate(c);
    c->proc_stream_time = stream_time_secs;
    c->proc_stream_status = stream_status;
    if (stream_status & 2u) c->n_underflows++;
    if (stream_status & 1u) c->n_overflows++;
    a.bytes[slot] = out_bytes;
    a.zeros[slot] = !c->have_plan || frames == 0;  // processor.rs:86-89 (Q19): no schedule yet -> silence
    if (!a.zeros[slot]) {
        if (!a.copy_stream) HIPC(c, hipStreamCreateWithFlags(&a.copy_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            if (!a.ev_render[i]) HIPC(c, hipEventCreateWithFlags(&a.ev_render[i], hipEventDisableTiming));
            if (!a.ev_copy[i]) HIPC(c, hipEventCreateWithFlags(&a.ev_copy[i], hipEventDisableTiming));
        }
        // (the device-side output block exists only in the copy modes: in the default mode 3 nothing ever wrote it — ADVICE r5)
        static const int mode = getenv("FWGPU_ASYNC_MODE") ? atoi(getenv("FWGPU_ASYNC_MODE")) : 3;
        if ((mode != 3 && out_bytes > a.d[slot].cap) || out_bytes > a.hcap[slot]) {  // (first call of this size only; the slot is idle: nothing reads it)
            RtHold hold(c);
            HIPC(c, hipStreamSynchronize(c->stream));
            if (mode != 3) HIPC(c, a.d[slot].ensure_n("d_async_out", out_bytes));
            if (out_bytes > a.hcap[slot]) {
                // ORDINARY (cacheable) host memory, page-locked for the DMA engine: the copy back is an SDMA transfer that runs beside the
                // next ticket's kernels (a copy into pageable memory is a blit KERNEL: it queued behind them — measured, no overlap), and
                // the host's memcpy out of it runs at memory speed (out of hipHostMalloc memory it cost 0.3 ms per 1.5 MiB — measured)
                if (a.h[slot]) {
                    (void)hipHostUnregister(a.h[slot]);
                    free(a.h[slot]);
                }
                a.h[slot] = nullptr;
                a.hcap[slot] = 0;
                const size_t cap = (out_bytes + 4095) & ~(size_t)4095;
                void* m = nullptr;
                if (posix_memalign(&m, 4096, cap) != 0 || !m) return fail(c, FWGPU_ERR_DEVICE, "out of host memory for the output staging");
                memset(m, 0, cap);
                hipError_t e = hipHostRegister(m, cap, hipHostRegisterMapped);
                void* dp = nullptr;
                if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, m, 0);
                if (e != hipSuccess) {
                    free(m);
                    return hipfail(c, e, "hipHostRegister(output staging)");
                }
                a.h[slot] = m;
                a.h_dev[slot] = (float*)dp;
                a.hcap[slot] = cap;
            }
        }
        const float* d_in = nullptr;
        if (n_in_ch > 0 && input) {
            const size_t in_bytes = (size_t)frames * n_in_ch * sizeof(float);
            if (in_bytes > c->d_in_stage.cap) {
                HIPC(c, hipStreamSynchronize(c->stream));
                HIPC(c, c->d_in_stage.ensure_n("d_in_stage", in_bytes));
            }
            HIPC(c, hipMemcpyAsync(c->d_in_stage.p, input, in_bytes, hipMemcpyHostToDevice, c->stream));
            d_in = c->d_in_stage.as<float>();
        }
        // Where the frames cross PCIe (round 5, config 2, 1.5 MiB per call, same box; the synchronous call: 0.313 ms per step):
        //   3 (default)  the graph-output kernel writes the interleaved frames STRAIGHT into the mapped host staging: no copy at all
        //   2            a copy in the ctx stream behind the render: 0.310 (DMA engine) / 0.325 (blit kernel) — serial with the next render
        //   0            a copy on a stream of its own behind the render's event: 0.579 (DMA engine) / 0.388 (blit kernel, HSA_ENABLE_SDMA=0):
        //                the cross-stream hand-over costs more than the overlap gives
        float* const d_out = mode == 3 ? a.h_dev[slot] : a.d[slot].as<float>();
        const int rc = run_blocks(c, frames, d_in, (int)n_in_ch, d_out, (int)n_out_ch);
        if (rc) return rc;
        if (out_bytes) {
            if (mode == 3) {
                HIPC(c, hipEventRecord(a.ev_copy[slot], c->stream));
            } else if (mode == 2) {
                HIPC(c, hipMemcpyAsync(a.h[slot], a.d[slot].p, out_bytes, hipMemcpyDeviceToHost, c->stream));
                HIPC(c, hipEventRecord(a.ev_copy[slot], c->stream));
            } else {
                HIPC(c, hipEventRecord(a.ev_render[slot], c->stream));
                HIPC(c, hipStreamWaitEvent(a.copy_stream, a.ev_render[slot], 0));
                HIPC(c, hipMemcpyAsync(a.h[slot], a.d[slot].p, out_bytes, hipMemcpyDeviceToHost, a.copy_stream));
                HIPC(c, hipEventRecord(a.ev_copy[slot], a.copy_stream));
            }
        }
    }
    a.ret_ticket[slot] = c->ret_ticket;
    a.busy[slot] = true;
    return a.next++;
}
int fwgpu_process_interleaved_end(fwgpu_ctx* c, int64_t ticket, float* output) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    fwgpu_ctx::AsyncOut& a = c->ao;
    const int slot = (int)(ticket & 1);
    if (ticket < 0 || ticket != a.done || ticket >= a.next || !a.busy[slot])
        return fail(c, FWGPU_ERR_INVALID, "not the oldest ticket in flight (tickets are ended in the order they were begun)");
    const size_t n = a.bytes[slot];
    if (n && !output) return fail(c, FWGPU_ERR_INVALID, "output is null (the ticket stays in flight: end it with a buffer, or fwgpu_process_interleaved_cancel)");
    a.busy[slot] = false;
    a.done++;
    if (a.zeros[slot] || n == 0) {
        if (n) memset(output, 0, n);
        return 0;
    }
    // the copy back went out in `begin`, on its own stream behind the ticket's last launch: the ctx stream — which may be rendering
    // the NEXT ticket — is not waited for
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipEventSynchronize(a.ev_copy[slot]);
    if (e != hipSuccess) {
        memset(output, 0, n);  // "all output buffers MUST be filled" (core/node.rs:41-42)
        return hipfail(c, e, "copy back of a process_interleaved_begin ticket");
    }
    const auto t1 = std::chrono::steady_clock::now();
    memcpy(output, a.h[slot], n);
    a.prof_wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
    a.prof_copy_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t1).count();
    a.prof_calls++;
    c->ret_done_ticket.store(a.ret_ticket[slot], std::memory_order_release);  // what that call handed back is final
    return 0;
}
// Abandon tickets: every ticket in flight up to and including `ticket` is waited for and its slot released, no frames copied — a host
// that unwinds (a Rust `Ticket` dropped on an error path) must not leave `begin` refusing for ever after two.
int fwgpu_process_interleaved_cancel(fwgpu_ctx* c, int64_t ticket) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    fwgpu_ctx::AsyncOut& a = c->ao;
    if (ticket < a.done || ticket >= a.next) return fail(c, FWGPU_ERR_INVALID, "no such ticket in flight");
    int rc = 0;
    while (a.done <= ticket) {
        const int slot = (int)(a.done & 1);
        if (a.busy[slot] && !a.zeros[slot] && a.bytes[slot]) {
            const hipError_t e = hipEventSynchronize(a.ev_copy[slot]);  // the staging block is idle again only once its writer has ended
            if (e != hipSuccess) rc = hipfail(c, e, "waiting for a cancelled process_interleaved_begin ticket");
            c->ret_done_ticket.store(a.ret_ticket[slot], std::memory_order_release);
        }
        a.busy[slot] = false;
        a.done++;
    }
    return rc;
}
int fwgpu_proc_info(fwgpu_ctx* c, double* stream_time_secs, uint32_t* stream_status, uint64_t* output_underflows,
                    uint64_t* input_overflows) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (stream_time_secs) *stream_time_secs = c->proc_stream_time;
    if (stream_status) *stream_status = c->proc_stream_status;
    if (output_underflows) *output_underflows = c->n_underflows;
    if (input_overflows) *input_overflows = c->n_overflows;
    return 0;
}

// ---- headless stream: DataCallback::callback (cpal/lib.rs:378-449) without a device.  The caller plays the part of
// cpal: it names the instant of each callback on its own clock; the stream-time / underflow bookkeeping is the reference's.
struct fwgpu_stream {
    fwgpu_ctx* ctx;
    uint32_t n_in, n_out;
    double sample_rate_recip;      // :371
    bool have_first_instant;       // first_stream_instant.is_some()
    double first_stream_instant;
    double predicted_stream_secs;  // :373
    bool is_first_callback;        // :374
    uint64_t callbacks, underflows;
    double last_stream_time;
};
fwgpu_stream* fwgpu_stream_open(fwgpu_ctx* c, uint32_t num_in_channels, uint32_t num_out_channels) {
    if (!c || num_in_channels > 64 || num_out_channels > 64) return nullptr;
    fwgpu_stream* s = new (std::nothrow) fwgpu_stream;
    if (!s) return nullptr;
    s->ctx = c;
    s->n_in = num_in_channels;
    s->n_out = num_out_channels;
    s->sample_rate_recip = 1.0 / (double)c->sample_rate;
    s->have_first_instant = false;
    s->first_stream_instant = 0.0;
    s->predicted_stream_secs = 1.0;
    s->is_first_callback = true;
    s->callbacks = s->underflows = 0;
    s->last_stream_time = 0.0;
    return s;
}
void fwgpu_stream_close(fwgpu_stream* s) { delete s; }
int fwgpu_stream_callback(fwgpu_stream* s, float* output, uint64_t frames, double callback_instant_secs) {
    if (!s) return FWGPU_ERR_INVALID;
    double stream_time_secs;
    bool underflow = false;
    const double block_secs = (double)frames * s->sample_rate_recip;
    if (s->is_first_callback) {  // :393-400 (the first callback's instant is ignored)
        s->is_first_callback = false;
        s->predicted_stream_secs = block_secs;
        stream_time_secs = 0.0;
    } else if (s->have_first_instant) {  // :401-420
        stream_time_secs = callback_instant_secs - s->first_stream_instant;
        underflow = stream_time_secs > s->predicted_stream_secs;
        s->predicted_stream_secs = stream_time_secs + (block_secs * 1.2);
    } else {  // :421-426
        s->have_first_instant = true;
        s->first_stream_instant = callback_instant_secs;
        stream_time_secs = s->predicted_stream_secs;
        s->predicted_stream_secs += block_secs * 1.2;
    }
    s->callbacks++;
    if (underflow) s->underflows++;
    s->last_stream_time = stream_time_secs;
    const uint32_t status = underflow ? 2u : 0u;  // StreamStatus::OUTPUT_UNDERFLOW (core/node.rs:130)
    // :434-442 process_interleaved(&[], output, ...); no processor yet (:446-449) = no schedule: output.fill(0.0) — which
    // fwgpu_process_interleaved does itself (Q19)
    const int rc = fwgpu_process_interleaved(s->ctx, nullptr, output, s->n_in, s->n_out, frames, stream_time_secs, status);
    return rc < 0 ? rc : (int)status;
}
int fwgpu_stream_run(fwgpu_stream* s, float* output, uint64_t frames, uint32_t n_callbacks, double first_instant_secs,
                     double* elapsed_secs) {
    if (!s || !output) return FWGPU_ERR_INVALID;
    const double period = (double)frames * s->sample_rate_recip;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    for (uint32_t i = 0; i < n_callbacks; ++i) {
        rc = fwgpu_stream_callback(s, output, frames, first_instant_secs + (double)i * period);
        if (rc < 0) break;
    }
    if (elapsed_secs) *elapsed_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc < 0 ? rc : 0;
}
int fwgpu_stream_stats(fwgpu_stream* s, uint64_t* callbacks, uint64_t* underflows, double* last_stream_time_secs) {
    if (!s) return FWGPU_ERR_INVALID;
    if (callbacks) *callbacks = s->callbacks;
    if (underflows) *underflows = s->underflows;
    if (last_stream_time_secs) *last_stream_time_secs = s->last_stream_time;
    return 0;
}

int fwgpu_process_blocks_device_flags(fwgpu_ctx* c, uint32_t num_blocks, float* d_output, uint32_t n_out_ch, uint8_t* d_silence) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    AudioGate gate(c);
    if (!c->have_plan) return fail(c, FWGPU_ERR_INVALID, "no schedule: call fwgpu_update first");
    if (num_blocks == 0) return 0;
    if (n_out_ch > 64 || (n_out_ch && !d_output)) return fail(c, FWGPU_ERR_INVALID, "bad output (null, or more than 64 channels)");
    c->out_sil = d_silence;
    const int rc = run_blocks(c, (uint64_t)num_blocks * c->mbf, nullptr, 0, d_output, (int)n_out_ch);
    c->out_sil = nullptr;
    return rc;
}
int fwgpu_process_blocks_device(fwgpu_ctx* c, uint32_t num_blocks, float* d_output, uint32_t n_out_ch) {
    return fwgpu_process_blocks_device_flags(c, num_blocks, d_output, n_out_ch, nullptr);
}
int fwgpu_process_blocks_device_io(fwgpu_ctx* c, uint32_t num_blocks, const float* d_input, uint32_t n_in_ch, float* d_output, uint32_t n_out_ch,
                                   uint8_t* d_silence) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    AudioGate gate(c);
    if (!c->have_plan) return fail(c, FWGPU_ERR_INVALID, "no schedule: call fwgpu_update first");
    if (num_blocks == 0) return 0;
    if (n_in_ch > 64 || n_out_ch > 64 || (n_out_ch && !d_output)) return fail(c, FWGPU_ERR_INVALID, "bad stream buffers (null output, or more than 64 channels)");
    c->out_sil = d_silence;
    const int rc = run_blocks(c, (uint64_t)num_blocks * c->mbf, (d_input && n_in_ch) ? d_input : nullptr, (d_input && n_in_ch) ? (int)n_in_ch : 0, d_output,
                              (int)n_out_ch);
    c->out_sil = nullptr;
    return rc;
}

int fwgpu_bus_sum_ordered_flags(fwgpu_ctx* c, const float* const* d_parts, const uint8_t* const* d_silence, uint32_t n_parts, float* d_out,
                                uint8_t* d_out_silence, uint64_t n_floats, uint32_t frames_per_block, uint32_t n_channels) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    if (n_parts == 0 || n_parts > FW_MAX_BUS_PARTS || !d_parts || !d_out) return fail(c, FWGPU_ERR_INVALID, "1..64 partial buses");
    BusParts bp;
    bp.n = (int)n_parts;
    for (uint32_t r = 0; r < n_parts; ++r) {
        if (!d_parts[r] || ((uintptr_t)d_parts[r] & 15u)) return fail(c, FWGPU_ERR_INVALID, "partial bus null or not 16-byte aligned");
        bp.part[r] = d_parts[r];
    }
    for (uint32_t r = n_parts; r < FW_MAX_BUS_PARTS; ++r) bp.part[r] = nullptr;
    if ((uintptr_t)d_out & 15u) return fail(c, FWGPU_ERR_INVALID, "output not 16-byte aligned");
    uint32_t n_blocks = 0;
    if (d_silence) {
        if (frames_per_block == 0 || n_channels == 0) return fail(c, FWGPU_ERR_INVALID, "silence flags need the block geometry (frames, channels)");
        const uint64_t per = (uint64_t)frames_per_block * n_channels;
        n_blocks = (uint32_t)((n_floats + per - 1) / per);
    }
    LCHK(c, launch_bus_sum_ordered(c->stream, bp, d_silence, d_out, d_out_silence, (size_t)n_floats, n_blocks, frames_per_block, n_channels));
    return 0;
}
int fwgpu_bus_sum_ordered(fwgpu_ctx* c, const float* const* d_parts, uint32_t n_parts, float* d_out, uint64_t n_floats) {
    return fwgpu_bus_sum_ordered_flags(c, d_parts, nullptr, n_parts, d_out, nullptr, n_floats, 0, 0);
}

int fwgpu_synchronize(fwgpu_ctx* c) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HIPC(c, hipStreamSynchronize(c->stream));
    return 0;
}

// Level meters (K_METER): the records of blocks [first_block, first_block + n) of `node`, out[i * n_in + c].  Audio side: waits for the
// ctx stream, then copies from the node's ring in the ext pool (at most two pieces: the ring wraps once).
int64_t fwgpu_meter_read(fwgpu_ctx* c, int64_t node, uint64_t first_block, uint32_t num_blocks, fwgpu_meter_reading* out, uint64_t* blocks_done) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    AudioGate gate(c);
    const uint64_t done = c->blocks_done;
    if (blocks_done) *blocks_done = done;
    HIPC(c, hipStreamSynchronize(c->stream));
    const PlanImage::Meter* m = nullptr;
    if (c->have_plan)
        for (const PlanImage::Meter& x : c->meters)
            if (x.id == node) m = &x;
    if (!m) return fail(c, FWGPU_ERR_INVALID, "not a meter node of the installed plan");
    if (num_blocks == 0) return 0;
    if (!out) return fail(c, FWGPU_ERR_INVALID, "meter_read: null output with blocks requested");
    if (first_block + (uint64_t)m->ring < done) return fail(c, FWGPU_ERR_INVALID, "meter_read: first_block is older than the ring retains");
    if (first_block < m->first_block) return fail(c, FWGPU_ERR_INVALID, "meter_read: first_block is older than the meter's first plan");
    static_assert(sizeof(fwgpu_meter_reading) == sizeof(MeterRec), "fwgpu_meter_reading layout");
    const uint64_t exist = done > first_block ? done - first_block : 0;
    const uint32_t n = (uint32_t)std::min<uint64_t>(num_blocks, exist);  // (<= ring: first_block + ring >= done)
    const MeterRec* ring = (const MeterRec*)(c->d_ext.as<float>() + m->ext_off);
    const uint32_t s0 = (uint32_t)(first_block % m->ring);
    const uint32_t n0 = std::min<uint32_t>(n, m->ring - s0);
    if (n0) HIPC(c, hipMemcpyAsync(out, ring + (size_t)s0 * m->n_in, (size_t)n0 * m->n_in * sizeof(MeterRec), hipMemcpyDeviceToHost, c->stream));
    if (n > n0)
        HIPC(c, hipMemcpyAsync(out + (size_t)n0 * m->n_in, ring, (size_t)(n - n0) * m->n_in * sizeof(MeterRec), hipMemcpyDeviceToHost, c->stream));
    if (n) HIPC(c, hipStreamSynchronize(c->stream));
    return (int64_t)n;
}
// Spectrum meters (a K_METER created with two or more parameters): the same call for the node's second ring, out[(i * n_in + c) * B + b]
int64_t fwgpu_spectrum_read(fwgpu_ctx* c, int64_t node, uint64_t first_block, uint32_t num_blocks, float* out, uint64_t* blocks_done) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    AudioGate gate(c);
    const uint64_t done = c->blocks_done;
    if (blocks_done) *blocks_done = done;
    HIPC(c, hipStreamSynchronize(c->stream));
    const PlanImage::Meter* m = nullptr;
    if (c->have_plan)
        for (const PlanImage::Meter& x : c->meters)
            if (x.id == node && x.fft) m = &x;
    if (!m) return fail(c, FWGPU_ERR_INVALID, "not a spectrum meter node of the installed plan");
    if (num_blocks == 0) return 0;
    if (!out) return fail(c, FWGPU_ERR_INVALID, "spectrum_read: null output with blocks requested");
    if (first_block + (uint64_t)m->ring < done) return fail(c, FWGPU_ERR_INVALID, "spectrum_read: first_block is older than the ring retains");
    if (first_block < m->first_block) return fail(c, FWGPU_ERR_INVALID, "spectrum_read: first_block is older than the meter's first plan");
    const uint64_t exist = done > first_block ? done - first_block : 0;
    const uint32_t n = (uint32_t)std::min<uint64_t>(num_blocks, exist);  // (<= ring: first_block + ring >= done)
    const float* ring = c->d_ext.as<float>() + m->spec_off;
    const size_t blk = (size_t)m->n_in * m->rec;  // floats of one block's records
    const uint32_t s0 = (uint32_t)(first_block % m->ring);
    const uint32_t n0 = std::min<uint32_t>(n, m->ring - s0);
    if (n0) HIPC(c, hipMemcpyAsync(out, ring + (size_t)s0 * blk, (size_t)n0 * blk * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (n > n0) HIPC(c, hipMemcpyAsync(out + (size_t)n0 * blk, ring, (size_t)(n - n0) * blk * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (n) HIPC(c, hipStreamSynchronize(c->stream));
    return (int64_t)n;
}
int fwgpu_spectrum_layout(fwgpu_ctx* c, int64_t node, uint32_t* fft_size, uint32_t* bands, uint32_t* edges, uint32_t edges_cap) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    AudioGate gate(c);
    const PlanImage::Meter* m = nullptr;
    if (c->have_plan)
        for (const PlanImage::Meter& x : c->meters)
            if (x.id == node && x.fft) m = &x;
    if (!m) return fail(c, FWGPU_ERR_INVALID, "not a spectrum meter node of the installed plan");
    if (fft_size) *fft_size = m->fft;
    if (bands) *bands = m->bands;
    if (edges && edges_cap) {
        std::vector<uint32_t> e((size_t)m->rec + 1);
        spectrum_edges(m->fft, m->bands, e.data());
        for (uint32_t b = 0; b < edges_cap && b <= m->rec; ++b) edges[b] = e[b];
    }
    return (int)m->rec;
}

int fwgpu_node_process(fwgpu_ctx* c, int64_t node, uint64_t frames, const float* const* inputs, uint32_t n_in,
                       float* const* outputs, uint32_t n_out, uint64_t in_mask, uint64_t* out_mask, double, uint32_t) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    AudioCallScope audio;
    use_device(c);
    AudioGate gate(c);
    { const int prc = rt_persist_stop(c); if (prc) return prc; }
    { const int prc = lazy_flush(c); if (prc) return prc; }  // (this node's state may lag behind lazily rendered blocks)
    // the node as the ACTIVE plan knows it (the graph belongs to the control thread, which may be editing it right now:
    // Firewheel activates and deactivates nodes while the audio thread is inside process(), graph.rs:586-612)
    const uint32_t nslot = (uint32_t)(node & 0xffffffff);
    const int pidx = (c->have_plan && nslot < c->slot_index.size()) ? c->slot_index[nslot] : -1;
    if (pidx < 0 || nslot >= c->slot_ids.size() || c->slot_ids[nslot] != node)
        return fail(c, FWGPU_ERR_INVALID, "node is not activated (call fwgpu_update)");
    const PlanNode* hn = &c->plan.nodes[pidx];
    if ((uint32_t)hn->n_in != n_in || (uint32_t)hn->n_out != n_out) return fail(c, FWGPU_ERR_INVALID, "port counts differ from add_node");
    if (frames > c->mbf) return fail(c, FWGPU_ERR_INVALID, "frames > max_block_frames");
    if (hn->kind == K_FIR) return fail(c, FWGPU_ERR_INVALID, "FIR banks run at graph level (fwgpu_process_interleaved), not per node");
    if (hn->kind == K_HOST) return fail(c, FWGPU_ERR_INVALID, "a host node's processor lives in the caller: call it there");
    if (n_in + n_out == 0) return fail(c, FWGPU_ERR_INVALID, "node has no ports");
    if (frames == 0) {  // the reference never calls a node with an empty block (processor.rs:86-89 returns first): nothing to do
        if (out_mask) *out_mask = 0;
        return 0;
    }
    if ((n_in && !inputs) || (n_out && !outputs)) return fail(c, FWGPU_ERR_INVALID, "null channel table");
    for (uint32_t i = 0; frames && i < n_in; ++i)
        if (!inputs[i]) return fail(c, FWGPU_ERR_INVALID, "null input channel");
    for (uint32_t i = 0; frames && i < n_out; ++i)
        if (!outputs[i]) return fail(c, FWGPU_ERR_INVALID, "null output channel");
    const size_t stride = (size_t)c->stride;
    const int nb = 1 + (int)n_in + (int)n_out;
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, c->d_scratch_pool.ensure_n("d_scratch_pool", (size_t)nb * stride * sizeof(float)));
    HIPC(c, c->d_scratch_flags.ensure_n("d_scratch_flags", (size_t)nb));
    HIPC(c, hipMemsetAsync(c->d_scratch_pool.p, 0, stride * sizeof(float), c->stream));
    uint8_t fl[1 + 64 + 64] = {0};  // (at most 64 ports per side)
    fl[0] = 1;
    for (uint32_t i = 0; i < n_in; ++i) {
        fl[1 + i] = (in_mask >> i) & 1ull;
        HIPC(c, hipMemcpyAsync(c->d_scratch_pool.as<float>() + (1 + i) * stride, inputs[i], frames * sizeof(float),
                               hipMemcpyHostToDevice, c->stream));
    }
    for (uint32_t i = 0; i < n_out; ++i)  // nodes that leave outputs untouched (dummy.rs, beep_test.rs:83-86)
        HIPC(c, hipMemcpyAsync(c->d_scratch_pool.as<float>() + (1 + n_in + i) * stride, outputs[i], frames * sizeof(float),
                               hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->d_scratch_flags.p, fl, nb, hipMemcpyHostToDevice, c->stream));
    // temp tables: [NodeDesc][in ids][out ids]
    int tab[sizeof(NodeDesc) / sizeof(int) + 64 + 64 + 2] = {0};
    const size_t tab_ints = sizeof(NodeDesc) / sizeof(int) + n_in + n_out + 2;
    NodeDesc nd;
    memset(&nd, 0, sizeof(nd));
    nd.kind = hn->kind;
    nd.n_in = (int)n_in;
    nd.n_out = (int)n_out;
    nd.in_off = 0;
    nd.out_off = 0;
    nd.state = (int)(node & 0xffffffff);
    nd.aux0 = (hn->kind == K_SUM && n_out) ? (int)(n_in / n_out) : 0;
    memcpy(tab, &nd, sizeof(nd));
    int* ins = tab + sizeof(NodeDesc) / sizeof(int);
    int* outs = ins + n_in + 1;
    for (uint32_t i = 0; i < n_in; ++i) ins[i] = 1 + (int)i;
    for (uint32_t i = 0; i < n_out; ++i) outs[i] = 1 + (int)n_in + (int)i;
    HIPC(c, c->d_scratch_tab.ensure_n("d_scratch_tab", tab_ints * sizeof(int)));
    HIPC(c, hipMemcpyAsync(c->d_scratch_tab.p, tab, tab_ints * sizeof(int), hipMemcpyHostToDevice, c->stream));
    int rc = upload_sample_table(c);
    if (rc) return rc;
    if ((rc = join_streams(c))) return rc;  // (a control-ahead call may still be in flight: one node, the main stream)
    c->cmds_on_ctl = false;
    rc = upload_cmds(c);
    if (rc) return rc;
    DevView v = generic_view(c, (int)frames);
    v.nodes = (const NodeDesc*)c->d_scratch_tab.p;
    v.in_buf = c->d_scratch_tab.as<int>() + sizeof(NodeDesc) / sizeof(int);
    v.out_buf = v.in_buf + n_in + 1;
    v.pool = c->d_scratch_pool.as<float>();
    v.flags = c->d_scratch_flags.as<uint8_t>();
    c->epoch++;
    v.gain_rides = hn->kind == K_VOLUME || hn->kind == K_PAN ? 1 : 0;  // (k_single_node<false, true>: CMD_GAIN_RIDE and a ride's blocks)
    v.sp_moves = hn->kind == K_SPATIAL ? 1 : 0;  // (k_single_node_spm: the build that takes CMD_SP_MOVE and renders a move)
    LCHK(c, launch_single_node(c->stream, v, 0));
    for (uint32_t i = 0; i < n_out; ++i)
        HIPC(c, hipMemcpyAsync(outputs[i], c->d_scratch_pool.as<float>() + (1 + n_in + i) * stride, frames * sizeof(float),
                               hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(fl, c->d_scratch_flags.p, nb, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    uint64_t om = 0;
    for (uint32_t i = 0; i < n_out; ++i)
        if (fl[1 + n_in + i]) om |= 1ull << i;
    if (out_mask) *out_mask = om;
    retire_cmds_node(c, (int)(node & 0xffffffff));
    return 0;
}

int fwgpu_timing_enable(fwgpu_ctx* c, int on) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    c->timing = on != 0;
    return 0;
}
int fwgpu_timing_read(fwgpu_ctx* c, int which, double* total_ms, uint64_t* launches) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    if (which < 0 || which > 4) return fail(c, FWGPU_ERR_INVALID, "timer index");
    timer_drain(c);
    *total_ms = c->timers[which].acc_ms;
    *launches = c->timers[which].launches;
    return 0;
}
int fwgpu_timing_reset(fwgpu_ctx* c) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    timer_drain(c);
    for (TimerCat& t : c->timers) {
        t.acc_ms = 0.0;
        t.launches = 0;
    }
    return 0;
}
#ifdef FW_DEBUG_BUS
// debugging builds only (make EXTRA=-DFW_DEBUG_BUS; scripts/dbg_rt.py — how round 4 found the leaf-bus store hazard): the fused plan's
// mix buses of block 0 of the last call, [n_bus][stride] floats
int fwgpu_debug_read_bus(fwgpu_ctx* c, float* out, uint64_t max_floats) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    (void)rt_persist_stop(c);
    HIPC(c, hipStreamSynchronize(c->stream));
    if (!c->d_bus.p) return fail(c, FWGPU_ERR_INVALID, "no fused plan");
    const uint64_t n = std::min<uint64_t>(max_floats, (uint64_t)c->n_bus * c->stride);
    HIPC(c, hipMemcpy(out, c->d_bus.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return (int)c->n_bus;
}
#endif
#ifdef FW_CHAIN_TRACE
// profiling builds only (scripts/chain_trace.py): timestamps [step 0..63][wave 0..15][slot 0..7] of workgroup 0
int fwgpu_debug_read_trace(fwgpu_ctx* c, unsigned long long* out) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    HIPC(c, hipStreamSynchronize(c->stream));
    if (!c->d_trace.p) return fail(c, FWGPU_ERR_INVALID, "no trace");
    HIPC(c, hipMemcpy(out, c->d_trace.p, 64 * 16 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}
#endif

int fwgpu_device_info(fwgpu_ctx* c, char* name, int name_cap, int* cus, uint64_t* hbm) {
    NEED_CTX(c, FWGPU_ERR_INVALID);
    hipDeviceProp_t prop;
    HIPC(c, hipGetDeviceProperties(&prop, c->device));
    if (name && name_cap > 0) {
        strncpy(name, prop.name[0] ? prop.name : prop.gcnArchName, (size_t)name_cap - 1);  // no marketing name: the ISA
        name[name_cap - 1] = 0;
    }
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm) *hbm = (uint64_t)prop.totalGlobalMem;
    return 0;
}

}  // extern "C"

#ifdef FW_PROBE
// scripts/placement_probe.py builds only (make EXTRA=-DFW_PROBE): exchange one device table between two contexts that hold
// the same graph — which table's place in HBM carries k_leaf_sum's slow / fast state?  Never part of a shipped library.
extern "C" int fwgpu_probe_swap(fwgpu_ctx* a, fwgpu_ctx* b, int which) {
    auto sw = [](DevBuf& x, DevBuf& y) {
        std::swap(x.p, y.p);
        std::swap(x.cap, y.cap);
    };
    switch (which) {
        case 0: sw(a->d_bus, b->d_bus); sw(a->d_bus_flags, b->d_bus_flags); break;
        case 1: sw(a->d_refs, b->d_refs); break;
        case 2: sw(a->d_gsets, b->d_gsets); break;
        case 3: sw(a->d_leaves, b->d_leaves); break;
        case 4: sw(a->d_samples, b->d_samples); break;
        case 5: sw(a->d_voices, b->d_voices); sw(a->d_blks, b->d_blks); sw(a->d_cache, b->d_cache); break;
        case 6: sw(a->d_ramps, b->d_ramps); break;
        default: return -1;
    }
    return 0;
}
#endif
