/* fwgpu.h — C ABI of libfwgpu: the MI355X (gfx950) per-block DSP executor for Firewheel audio graphs.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no C++/torch types.
 * Each entry point names the reference interface (BillyDM/firewheel @ 2024-10-16) it replaces:
 *   core/  = crates/firewheel-core/src/      graph/ = crates/firewheel-graph/src/
 *   nodes/ = crates/firewheel-graph/src/basic_nodes/
 *
 * Conventions (replacing Rust's Result/panic, SURVEY §8b "error convention"):
 *   - functions return int: 0 = ok, negative = error; handles are int64 (>= 0) or negative error.
 *   - nothing throws or aborts across the ABI; fwgpu_last_error() returns the message.
 *   - threading: a ctx has an AUDIO side — fwgpu_process_interleaved / _process_blocks_device[_flags] /
 *     _node_process / _stream_callback, one thread at a time — and a CONTROL side, everything else, ALSO one thread at a
 *     time (a host with several control threads serialises them itself: a message call looks its node up in the graph a
 *     graph call may be growing).  Every control call may run WHILE a process call is in flight:
 *       * messages (fwgpu_node_set_param, fwgpu_sampler_*) go through a lock-free ring the audio side drains at the start
 *         of its next call (the reference's Arc<AtomicF32> gains and rtrb rings: nodes/volume.rs:10,28-34,
 *         nodes/sampler.rs:14,171-177,205-208);
 *       * graph calls (add_node / remove_node / connect / disconnect / host_node_set_process / update / schedule_upload):
 *         update BUILDS the new plan off to the side on the calling thread and the next process call adopts it at its
 *         start, as the reference hands a new schedule over through a ring (graph/processor.rs:167-206;
 *         fwgpu_plan_handover_stats) — the audio side neither locks nor allocates nor waits for the build;
 *       * sample-table and configuration calls (sample_create / sample_destroy / set_force_generic) upload their data first
 *         and then hold process calls at their ENTRY for the few microseconds the table entry takes (they wait for a
 *         running call to finish first).  fwgpu_set_max_batch takes effect with the next update.
 *   - once warm, a process call touches neither the host allocator nor the device allocator; a failing call writes its
 *     message into a fixed buffer.  fwgpu_process_interleaved fills `output` on EVERY return (zeros on error:
 *     core/node.rs:41-42).
 *   - the library fails loudly (ctx_create returns NULL) when no HIP device / kernel image is usable;
 *     there is no CPU fallback anywhere behind this ABI.
 */
#ifndef FWGPU_H
#define FWGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fwgpu_ctx fwgpu_ctx;

/* node kinds — nodes/mod.rs:1-15 plus the north-star nodes the reference lists as TODO (README.md:14-19) */
enum fwgpu_node_kind {
    FWGPU_DUMMY = 0,          /* nodes/dummy.rs */
    FWGPU_BEEP_TEST = 1,      /* nodes/beep_test.rs   params: freq_hz, gain_db, enabled */
    FWGPU_VOLUME = 2,         /* nodes/volume.rs      params: percent_volume */
    FWGPU_SUM = 3,            /* nodes/sum.rs */
    FWGPU_SAMPLER = 4,        /* nodes/sampler.rs     params: percent_volume */
    FWGPU_HARD_CLIP = 5,      /* nodes/hard_clip.rs   params: threshold_db */
    FWGPU_MONO_TO_STEREO = 6, /* nodes/mono_to_stereo.rs */
    FWGPU_STEREO_TO_MONO = 7, /* nodes/stereo_to_mono.rs */
    FWGPU_STEREO_PAN = 8,     /* SPEC (not in reference) params: pan in [-1,1] */
    FWGPU_STEREO_WIDTH = 9,   /* SPEC                 params: width */
    FWGPU_BIQUAD = 10,        /* SPEC                 params: type, cutoff_hz, q */
    FWGPU_DELAY = 11,         /* SPEC                 params: delay_secs, feedback, mix */
    FWGPU_FIR = 12,           /* SPEC convolution     params: impulse-response sample id (fwgpu_sample_create).  With two or more
                                 parameters the node is morph-capable: ir_a, ir_b (-1: empty), max_taps (0: the longer of the two),
                                 position (0..1, default 0), law (0 linear, 1 equal power; default 1); see "FIR morph" below */
    FWGPU_RESAMPLER = 13,     /* SPEC polyphase resampling source (0 inputs)  params: sample id, ratio, loop, playing */
    FWGPU_SPATIAL = 14,       /* SPEC 3D spatialiser (1|2 in, 2 out)          params: x, y, z of the source */
    FWGPU_HOST_NODE = 15,     /* any other `dyn AudioNodeProcessor` (graph/processor.rs:243): runs on the HOST, see below */
    FWGPU_METER = 16,         /* SPEC level meter     params: ring_blocks (1..65536, default 1024); see fwgpu_meter_read.  With two or more
                                 parameters a spectrum meter: ring_blocks, fft_size, bands; see fwgpu_spectrum_read */
    FWGPU_LIMITER = 17,       /* SPEC look-ahead limiter (n in, n out, n in 1..8)  params: ceiling (linear, 0.001..1000, default 1.0),
                                 hold_frames (0..1920, default 128); see FWGPU_LIMITER_LATENCY */
    FWGPU_DUCKER = 18,        /* SPEC sidechain ducker (n + k in, n out, n and k in 1..8)  params: threshold (linear, 1e-6..1000, default
                                 0.05), depth (0..1, default 0.25), attack_frames (1..32768, default 480), release_frames (1..32768,
                                 default 12000), hold_frames (0..32768, default 4800); see "sidechain ducker" below */
    FWGPU_DELAY_COMP = 19,    /* SPEC latency compensation (n in, n out, n in 1..8)  params: frames (a whole number in
                                 0..FWGPU_DELAY_COMP_MAX, default 63); see "latency compensation" below */
    FWGPU_CROSSFADE = 20,     /* SPEC crossfader (2n in, n out, n in 1..8)  params: position (0..1, default 0 = all of bus A), law
                                 (0 linear, 1 equal power; default 1); see "crossfader" below and fwgpu_crossfade_to */
    FWGPU_COMPRESSOR = 21     /* SPEC bus compressor (n in, n out, n in 1..8)  params: threshold (linear, 1e-6..1000, default 0.25), ratio
                                 (1..1000, default 4), knee_db (full width, 0..24, default 6), attack_frames (1..32768, default 240),
                                 release_frames (1..32768, default 12000), hold_frames (0..2048, default 0), makeup (linear,
                                 0.001..1000, default 1.0); see "bus compressor" below */
};

/* sample formats — core/sample_resource.rs:28-335 */
enum fwgpu_sample_format {
    FWGPU_INTERLEAVED_I16 = 0,
    FWGPU_INTERLEAVED_U16 = 1,
    FWGPU_INTERLEAVED_F32 = 2,
    FWGPU_PLANAR_I16 = 3, /* data = channels planes of `frames` items, concatenated */
    FWGPU_PLANAR_U16 = 4,
    FWGPU_PLANAR_F32 = 5
};

/* error codes: AddEdgeError / CompileGraphError variants (graph/graph/error.rs) */
enum fwgpu_error {
    FWGPU_OK = 0,
    FWGPU_ERR_SRC_NODE_NOT_FOUND = -1,
    FWGPU_ERR_DST_NODE_NOT_FOUND = -2,
    FWGPU_ERR_IN_PORT_OUT_OF_RANGE = -3,
    FWGPU_ERR_OUT_PORT_OUT_OF_RANGE = -4,
    FWGPU_ERR_EDGE_ALREADY_EXISTS = -5,
    FWGPU_ERR_INPUT_PORT_ALREADY_CONNECTED = -6,
    FWGPU_ERR_CYCLE_DETECTED = -7,
    FWGPU_ERR_COMPILE_CYCLE = -10,
    FWGPU_ERR_COMPILE_MANY_TO_ONE = -11,
    FWGPU_ERR_NODE_ACTIVATION_FAILED = -12,
    FWGPU_ERR_INVALID = -20,   /* bad handle / argument */
    FWGPU_ERR_QUEUE_FULL = -21,/* sampler message ring full (nodes/sampler.rs:14 CHANNEL_CAPACITY) */
    FWGPU_ERR_DEVICE = -30     /* HIP error; see fwgpu_last_error */
};

/* ---- context: FirewheelGraphCtx::new + activate (graph/context.rs:35-82) and the device-resident
 * FirewheelProcessor (graph/processor.rs:34-55).  `hip_stream` may be NULL (the ctx creates its own
 * stream) or a hipStream_t the caller owns (e.g. torch's current stream). */
fwgpu_ctx* fwgpu_ctx_create(int device, uint32_t sample_rate, uint32_t max_block_frames,
                            uint32_t num_graph_inputs, uint32_t num_graph_outputs, void* hip_stream);
void fwgpu_ctx_destroy(fwgpu_ctx* ctx);
const char* fwgpu_last_error(fwgpu_ctx* ctx);
/* message of the last failed fwgpu_ctx_create (which has no ctx to ask) */
const char* fwgpu_create_error(void);

/* ---- graph edit API: AudioGraph (graph/graph.rs) */
int64_t fwgpu_graph_in_node(fwgpu_ctx* ctx);  /* graph.rs:189 */
int64_t fwgpu_graph_out_node(fwgpu_ctx* ctx); /* graph.rs:194 */
/* graph.rs:201-231 add_node(num_inputs, num_outputs, node); `params` are the node constructor args */
int64_t fwgpu_add_node(fwgpu_ctx* ctx, int kind, uint32_t num_inputs, uint32_t num_outputs,
                       const float* params, int n_params);
int fwgpu_remove_node(fwgpu_ctx* ctx, int64_t node); /* graph.rs:268-299 */
/* graph.rs:396-477; returns the edge id or an AddEdgeError code */
int64_t fwgpu_connect(fwgpu_ctx* ctx, int64_t src_node, uint32_t src_port, int64_t dst_node,
                      uint32_t dst_port, int check_for_cycles);
int fwgpu_disconnect(fwgpu_ctx* ctx, int64_t src_node, uint32_t src_port, int64_t dst_node,
                     uint32_t dst_port);                 /* graph.rs:483-501; 1 = removed, 0 = no such edge */
int fwgpu_disconnect_edge(fwgpu_ctx* ctx, int64_t edge); /* graph.rs:507-524 */
int fwgpu_cycle_detected(fwgpu_ctx* ctx);                /* graph.rs:573-580 */
/* FirewheelGraphCtx::update (graph/context.rs:93-137): recompile when dirty, activate new nodes
 * (AudioNode::activate, core/node.rs:12-18), build + upload the device launch plan. */
int fwgpu_update(fwgpu_ctx* ctx);

/* ---- custom nodes inside a device-resident graph ("unknown/custom Rust nodes fall back to B1 on host with explicit
 * D2H/H2D of just their buffers").  The reference calls ANY `dyn AudioNodeProcessor` from its schedule loop
 * (graph/processor.rs:226-247); a node this library has no kernel for is added as FWGPU_HOST_NODE with its port counts and
 * given its process function — `AudioNodeProcessor::process` + `ProcInfo` (core/node.rs:37-53,94-118) as a C callback:
 * inputs[i] / outputs[i] are `frames` floats, in_silence_mask bit i = input i is silent, *out_silence_mask arrives 0
 * (processor.rs:233), every output must be filled.  The launch plan is CUT at such a node's level: the levels above it run on
 * the device, its input buffers (and only those) are copied to pinned host memory, the callback runs on the AUDIO thread —
 * once per block, in block order, like the reference — its outputs go back, the levels below continue.  A process call of K
 * blocks crosses the boundary twice per host level, not twice per block.  Voice banks of the graph stay on the fused kernels
 * (hybrid plan).  The function must be set before the fwgpu_update / fwgpu_schedule_upload that activates the node; it must
 * not call back into this ctx. */
typedef void (*fwgpu_host_process_fn)(void* user, uint64_t frames, const float* const* inputs, uint32_t num_inputs,
                                      float* const* outputs, uint32_t num_outputs, uint64_t in_silence_mask,
                                      uint64_t* out_silence_mask, double stream_time_secs, uint32_t stream_status);
int fwgpu_host_node_set_process(fwgpu_ctx* ctx, int64_t node, fwgpu_host_process_fn fn, void* user);
/* how many host nodes the installed plan holds / how often their callbacks have run since the plan was installed */
int fwgpu_plan_host_nodes(fwgpu_ctx* ctx, uint64_t* callbacks_run);

/* ---- external schedule import: keep Firewheel's own Rust scheduler and hand its CompiledSchedule over
 * (graph/graph/compiler/schedule.rs:12-30,105-126,166-173).  Buffer indices are the reference's; the
 * library reconstructs the edges, renames buffers (no reuse inside a level) and levelises. */
typedef struct fwgpu_sched_node {
    int64_t node;                 /* id returned by fwgpu_add_node / graph_in / graph_out */
    uint32_t num_inputs;
    uint32_t num_outputs;
    const uint32_t* in_buffer_index;  /* [num_inputs]  InBufferAssignment.buffer_index */
    const uint8_t* in_should_clear;   /* [num_inputs]  InBufferAssignment.should_clear */
    const uint32_t* out_buffer_index; /* [num_outputs] OutBufferAssignment.buffer_index */
} fwgpu_sched_node;
int fwgpu_schedule_upload(fwgpu_ctx* ctx, const fwgpu_sched_node* nodes, uint32_t n_nodes,
                          uint32_t num_buffers);

/* ---- introspection of the device launch plan (tests) */
/* 0 = generic level-batched executor, 1 = fused voice-bank plan (k_leaf_sum),
 * 2 = fused chain plan (voices with a biquad / delay: k_chain), 3 = hybrid: voice banks inside a graph that is not a fused
 * shape as a whole (sends, bus effects, anything) are rendered by the voice-bank kernels, the rest by the level executor */
int fwgpu_plan_kind(fwgpu_ctx* ctx);
/* how many voices (source -> stages chains) of the installed plan the fused kernels render — all of them on plans 1 and 2,
 * the banks' on plan 3, 0 on plan 0; -1 without a plan */
int fwgpu_plan_fused_voices(fwgpu_ctx* ctx);
int fwgpu_plan_num_levels(fwgpu_ctx* ctx);
/* level of a node in the plan (graph_in = 0); negative if unknown */
int fwgpu_plan_node_level(fwgpu_ctx* ctx, int64_t node);
/* per input port: 1 if the port is unconnected (the reference's should_clear), else 0.  Returns n. */
int fwgpu_plan_node_inputs_clear(fwgpu_ctx* ctx, int64_t node, int* should_clear, int cap);
/* chain plan (kind 2) only: k_chain workgroup launches since the plan was installed that ran the steady-call loop
 * (every voice of the leaf steady for the whole call, delays >= 3 tiles, no message pending) / the general loop */
int fwgpu_plan_chain_stats(fwgpu_ctx* ctx, uint64_t* steady_workgroups, uint64_t* general_workgroups);
/* Plan hand-over (graph/context.rs:93-137 + graph/processor.rs:167-206).  fwgpu_update / fwgpu_schedule_upload BUILD the new
 * plan on the calling (control) thread, off to the side, while process calls keep running on the current one; the next process
 * call adopts it at its start — a swap of descriptors plus a handful of asynchronous launches for the nodes it activates, no
 * allocation, no wait for the device — and the old plan travels back to the control side, whose next update reuses its
 * buffers.  (When no process call is in flight the updating thread adopts the plan itself, right away.)  *adoptions = plans
 * adopted so far, *audio_adoptions = those a process call adopted, *max_adopt_ns = the longest one of THOSE held up its process
 * call (host nanoseconds).  Any pointer may be NULL. */
int fwgpu_plan_handover_stats(fwgpu_ctx* ctx, uint64_t* adoptions, uint64_t* audio_adoptions, uint64_t* max_adopt_ns);
/* 1 while a plan built by fwgpu_update / fwgpu_schedule_upload waits for a process call to adopt it, else 0.  Once an update has
 * returned and this reads 0, the plan it built is the active one: nothing the update removed — a host node's callback and its
 * `user` pointer above all — will be called again, and its owner may free it (the reference drops a removed node's processor when
 * the old schedule comes back through the ring, graph/processor.rs:182-188; rust/firewheel-gpu's HostNodeHandle and the Python
 * wrapper keep removed host nodes in limbo until this says so).  Any thread may ask. */
int fwgpu_plan_pending(fwgpu_ctx* ctx);
/* Voice-bank and chain plans, diagnostics: launch batches of process calls rendered WITHOUT a control kernel (*lazy_batches) and with one.
 * A message-free call of a plan whose every voice the last control kernel left steady and plain (silent, or a planar-f32 source
 * or interleaved 16-bit source that never wraps inside a block) needs no per-block state machine pass — the reference's processors do nothing in such a block
 * but advance a playhead (nodes/sampler.rs:445-484) — and the leaf kernel derives each block's record from one per-voice
 * record; the host skips the control kernel once it has SEEN (pinned memory) that the last one found every voice so.  A host that
 * never waits for the device between calls sees no difference but the time.  FWGPU_LAZY=0 switches it off.  Either may be NULL. */
int fwgpu_lazy_stats(fwgpu_ctx* ctx, uint64_t* lazy_batches, uint64_t* control_batches);
/* Voice-bank plans, diagnostics: launch batches since creation that ONE kernel rendered — leaves, root sum and interleave per
 * (block, 256-frame piece), the leaf sums never leaving the chip.  Only a batch counted in *lazy_batches above can be one, and only of a
 * plan whose mixer tree is leaves -> root -> stereo output, from a size up (FWGPU_LEAF_GROUP=0|1, read at creation, switches it;
 * FWGPU_LEAF_GROUP_MIN sets the smallest blocks x pieces).  The output is the same bit for bit either way.  May be NULL. */
int fwgpu_plan_group_stats(fwgpu_ctx* ctx, uint64_t* grouped_batches);
/* The hipStream_t every process call of this ctx launches on (the caller's, or the one fwgpu_ctx_create made): for callers that
 * order their own device work or events against the engine's (bench.py's per-step time distribution).  NULL ctx -> NULL. */
void* fwgpu_hip_stream(fwgpu_ctx* ctx);
/* Diagnostics for the same hand-over: which part of fwgpu_update / fwgpu_schedule_upload the control thread is in right now —
 * 0 none, 1 compiling the graph (host only: graph/compiler.rs), 21..28 the sections of the plan build that upload tables
 * (23 node tables, 26 buffer pool, 27 voice tables, 28 staging areas), 3 waiting for the last upload.  Any thread may ask;
 * examples/host_c/fw_edit_race.c tags every callback with it to say WHEN a build reaches the audio side. */
int fwgpu_update_phase(fwgpu_ctx* ctx);
/* Realtime edge, resident kernel (cpal/lib.rs:378-449: a backend thread that is woken per block, never torn down between blocks).
 * The first steady one-block fwgpu_process_interleaved call of a run of them — voice-bank plan, stereo stream, no message pending —
 * launches a kernel that stays resident and is handed every following callback through a doorbell word in pinned host memory: no
 * launch call on the audio thread, no grid dispatch.  Anything else that touches the device state (a call with a message, a call of
 * another size, a plan adoption, fwgpu_node_process, destroy) ends it first; its own WATCHDOG ends it after `idle_ms` without a
 * callback (default 20; FWGPU_RT_IDLE_MS), so it can never hold a device that nobody feeds — the next callback launches a new one.
 * FWGPU_RT_PERSIST=0 switches it off (every callback is then one k_rt_block launch).  *launches = resident kernels launched so far,
 * *doorbells = callbacks served without a launch.  Any pointer may be NULL. */
int fwgpu_rt_resident_stats(fwgpu_ctx* ctx, uint64_t* launches, uint64_t* doorbells);
/* Which path the ONE-BLOCK calls of this context took so far (cpal/lib.rs:429-437 calls once per block for every graph; only some
 * plans have the one-launch edge): paths[0] = the resident kernel's doorbell (no launch), paths[1] = one k_rt_block launch,
 * paths[2] = the fused plans' ordinary launch sequence (a chain plan, a spatialiser / master chain, a tree of more than two levels,
 * a call that carried a message), paths[3] = the level executor (generic / hybrid plans).  A host reads it to see that its
 * callbacks run where it expects them to. */
int fwgpu_rt_path_stats(fwgpu_ctx* ctx, uint64_t* paths);  /* paths: room for 4 */
/* K = the most blocks one fused launch sequence processes (default 64); sizes the K-batched descriptor,
 * ramp and bus buffers at the next fwgpu_update. */
int fwgpu_set_max_batch(fwgpu_ctx* ctx, uint32_t max_blocks);
/* force the generic executor even when the fused plan matches (parity tests) */
int fwgpu_set_force_generic(fwgpu_ctx* ctx, int on);
/* floats of the per-node extended state pool (delay rings, FIR history, filter state) handed out / allocated: removing
 * a node returns its slice for reuse, so a host that spawns and retires effect voices sees `in_use` level off */
int fwgpu_ext_pool_floats(fwgpu_ctx* ctx, uint64_t* in_use, uint64_t* capacity);

/* ---- sample resources: SampleResource (core/sample_resource.rs:4-26), uploaded once, HBM-resident.
 * Returns a sample id >= 0. */
int fwgpu_sample_create(fwgpu_ctx* ctx, int format, uint32_t channels, uint64_t frames, const void* data);
/* same, from memory that is already on this device (bench: generate in HBM, skip PCIe) */
int fwgpu_sample_create_device(fwgpu_ctx* ctx, int format, uint32_t channels, uint64_t frames,
                               const void* device_data);
/* Releases the sample's HBM (for an id from fwgpu_sample_create; a _device sample only loses its table entry).  The
 * reference keeps a sample alive through the Arc every processor holds; here the CALLER guarantees that no sampler
 * will read the id any more (the Rust shim calls this when the last Arc drops).  Waits for the work
 * in flight on the context's stream.  Ids are never reused.  A sampler that still holds the id plays an EMPTY
 * (0-frame) sample from the next process call on — silence, never a stale pointer; FIR / resampler nodes name their
 * sample at construction, so the call is refused (FWGPU_ERR_INVALID) while such a node exists. */
int fwgpu_sample_destroy(fwgpu_ctx* ctx, int sample);
/* ProcessorToNodeMsg::ReturnSample (nodes/sampler.rs:339-343,563-571): when a SetSample message replaces the sample a
 * sampler holds — or a sampler node is removed and its processor dropped — the processor hands the old one back to the
 * node, which is when the host may let go of it.  Here: every sample that a process call COMPLETED on the device has
 * swapped out since the last poll, oldest first, as (node id, sample id) pairs.  Control side, never blocks (it asks
 * the completion events, it does not wait for them).  Returns the number of pairs written (<= cap). */
int fwgpu_poll_returned_samples(fwgpu_ctx* ctx, int64_t* nodes, int* samples, int cap);
/* 1 when no sampler holds `sample`, no queued SetSample message names it, every process call that read it has completed
 * on the device and no FIR / resampler node was built on it — i.e. fwgpu_sample_destroy is safe and changes no sound;
 * 0 otherwise.  (The reference gets this from Arc's count reaching zero after the ReturnSample above.) */
int fwgpu_sample_retired(fwgpu_ctx* ctx, int sample);

/* ---- control -> audio messages.  `at_block` = index of the max_block_frames-sized block, counted from
 * the start of the NEXT process call, before which the message is seen (the reference's rings/atomics
 * are polled at block start: nodes/sampler.rs:331, nodes/volume.rs:92).  Messages to one node apply in (at_block, send) order.
 * Send a node's messages in NON-DECREASING at_block order: the reference has no tag at all — "message, then process" is the only
 * order it knows — and parameters the control side folds into derived state (a biquad's cutoff and Q into its five coefficients,
 * computed in f64 with the host's libm) are folded WHEN THE MESSAGE IS SENT, with the node's other parameters as last sent; out
 * of block order they take effect as sent, not as tagged (found by tests/test_chain_grammar.py's fuzz, round 6). */
/* VolumeNode::set_percent_volume (volume.rs:28-34) / SamplerNode::set_percent_volume (sampler.rs:171-177):
 * param 0.  BeepTestNode::set_enabled (beep_test.rs:30-32): param 0.  SPEC nodes: StereoPan 0 = pan;
 * StereoWidth 0 = width; Biquad 1 = cutoff_hz, 2 = q; Delay 1 = feedback, 2 = mix; Resampler 1 = ratio,
 * 3 = playing, 4 = seek (source frame); Spatial 0/1/2 = x/y/z; Crossfade 0 = position (a jump: fwgpu_crossfade_to with
 * frames 0). */
int fwgpu_node_set_param(fwgpu_ctx* ctx, int64_t node, int param, float value, uint32_t at_block);
/* The same for `n` messages in one call, in order (hosts behind a foreign-function interface pay per call: bench.py's variant B
 * issues a hundred per step).  Stops at the first message that fails and returns its (negative) error; the ones in front of it
 * stay sent.  0 = all sent. */
int fwgpu_node_set_params(fwgpu_ctx* ctx, uint32_t n, const int64_t* nodes, const int* params, const float* values, const uint32_t* at_blocks);
int fwgpu_sampler_set_sample(fwgpu_ctx* ctx, int64_t node, int sample, int stop_playback,
                             uint32_t at_block);                                  /* sampler.rs:67-79 */
int fwgpu_sampler_play(fwgpu_ctx* ctx, int64_t node, uint32_t at_block);  /* sampler.rs:82-97 */
int fwgpu_sampler_pause(fwgpu_ctx* ctx, int64_t node, uint32_t at_block); /* sampler.rs:100-115 */
int fwgpu_sampler_stop(fwgpu_ctx* ctx, int64_t node, uint32_t at_block);  /* sampler.rs:118-133 */
int fwgpu_sampler_set_playhead_secs(fwgpu_ctx* ctx, int64_t node, double playhead_secs,
                                    uint32_t at_block);                           /* sampler.rs:136-147 */
/* mode: 0 = None, 1 = LoopRange::Full, 2 = LoopRange::RangeSecs(start..end)  (sampler.rs:150-161) */
int fwgpu_sampler_set_loop_range(fwgpu_ctx* ctx, int64_t node, int mode, double start_secs,
                                 double end_secs, uint32_t at_block);

/* ---- sampler: a gain envelope per voice — declicked pause, stop and start in one message (SPEC).
 * fwgpu_sampler_fade: from the first frame of block `at_block` of the next process call, move the sampler's envelope to `target`
 * (0..1) over `frames` frames, linearly, and at the fade's end do `then`.  One CMD_SMP_FADE (16), ordered like every sampler message.
 * A sampler has an envelope E0, E1 (f32 in 0..1), N, k (integers, k < N <= 2^24) and `then`; it is at rest when N == 0, its value at
 * rest is E1, and a new sampler rests at 1.0f.  The value of the frame j frames ahead of the current position:
 *   env(j) = N == 0 || k + j >= N ? E1
 *          : clamp(E0 + (d * ((float)(k + j) / (float)N)), min(E0, E1), max(E0, E1))        d = E1 - E0, computed once
 * every operation a separately rounded f32 operation, the division IEEE, no FMA; (float)(k + j) and (float)N are exact.  env(0) of a
 * fresh fade is E0 bit for bit; the value is monotone in j and never leaves [min, max] (E0 + d can round one ulp past E1: the clamp).
 * The message, at a block's first frame: frames == 0: E1 = target, at rest, then = NONE.  Else E0 = env(0) under the old state (a
 * retarget in mid-fade continues from where the fade stands), E1 = target, N = frames, k = 0, `then` as given.
 * Rendering: the envelope moves with the gain smoother — in exactly the blocks in which the reference reaches
 * gain_smoother.set_and_process (sampler.rs:432: a sample is set and alive, the sampler is playing), whatever happens afterwards.  The
 * block's gains are g[i] = s[i] * env(i), one f32 product (s[i]: what the smoother gives, a constant or its ramp), the output x * g[i].
 * The mute test (sampler.rs:437) stays a test on the smoother alone; there is no new silence rule: a voice resting at 0 renders zeros.
 * Behind the block: k += frames; a fade in flight with k >= N is over (N = k = 0) and, for `then` PAUSE / STOP, the sampler does exactly
 * what fwgpu_sampler_pause / _stop at the next block's first frame would do — the block the fade ended in was rendered whole, its frames
 * behind the end at E1 — after which the envelope rests at 1.0f; with then == NONE it rests at E1.
 * The envelope is a transient: whenever `playing` goes false for any other reason — pause, stop, set_sample with stop_playback, a
 * one-shot that ends (behind that block's gains) — it goes to rest at 1.0f with then = NONE.  No other message touches it (play,
 * set_playhead, set_loop_range, set_percent_volume, set_sample without stop): a level that should last belongs in percent_volume.
 * Without a fade message nothing changes by a bit (s * 1.0f == s).  A fade-in of a stopped voice is three messages for one block:
 * fade(0, 0), play, fade(1, N).  A voice inside a fade is not steady: its calls run the control kernel, and lazy calls resume behind
 * the fade.  Resampling sources (FWGPU_RESAMPLER) have no envelope.
 * FWGPU_ERR_INVALID: `node` is no FWGPU_SAMPLER; `target` is NaN, infinite or outside 0..1 (-0.0 counts as +0.0); frames >
 * FWGPU_SAMPLER_FADE_FRAMES_MAX; `then` outside 0..2; frames == 0 with then != FWGPU_FADE_NONE (a step has no end to wait for: use
 * fwgpu_sampler_stop).  FWGPU_ERR_QUEUE_FULL as the other sampler messages.  A fade for a node no plan holds yet waits for the update. */
enum fwgpu_fade_then { FWGPU_FADE_NONE = 0, FWGPU_FADE_PAUSE = 1, FWGPU_FADE_STOP = 2 };
#define FWGPU_SAMPLER_FADE_FRAMES_MAX 16777216
int fwgpu_sampler_fade(fwgpu_ctx* ctx, int64_t node, float target, uint32_t frames, int then, uint32_t at_block);

/* ---- streaming sample sources: a sampler that plays a ring fed while it plays (SPEC; the "disk and network streaming"
 * of the reference's DESIGN_DOC.md:11-28).  A stream is a sample whose storage is a ring of R = ring_frames frames, zeroed at creation.
 * The control side appends frames to it, ONE sampler plays them in order; a block for which the frames are not there yet is silent, and
 * the voice carries on in the block in which they are.  The id lives in the sample table like any other: fwgpu_sample_destroy and
 * fwgpu_sample_retired work on it unchanged.  All six formats; R in [4 * max_block_frames, 2^30], anything else is FWGPU_ERR_INVALID.
 * A stream that is never starved needs a ring that holds a whole process call: R >= (blocks per call + 1) * max_block_frames.
 *   write         accepts min(frames, R - (written - consumed_seen)) frames and returns that number.  consumed_seen is the consumed count
 *                 of the last process call KNOWN to be complete: it lags the device, so the free space is an underestimate, never an
 *                 overestimate.  `data` is laid out as fwgpu_sample_create lays out a sample of `frames` frames (planar: channel c starts
 *                 c * frames elements in).  The frames go straight into the free part of the ring (split at its end, and per channel for
 *                 the planar formats) by plain copies on a stream of the control side's own — never the audio stream, never waiting for
 *                 a process call — and once they have landed ONE message (CMD_SMP_STREAM = 17, at_block 0) tells the bound sampler the
 *                 new `written`: the frames can be played from the first block of the next process call, and no frame is read before it
 *                 is there.  A full message ring: `written` does not move, FWGPU_ERR_QUEUE_FULL, and the same call can be repeated.
 *                 Writes before a sampler holds the stream only fill the ring.
 *   write_device  the same from memory already on this device (a decoder on the GPU, a torch tensor).
 *   end           appends max_block_frames frames of padding behind the data (zero bytes; 0x8000 for the unsigned 16-bit formats, which
 *                 have no element that decodes to 0.0) and tells the sampler E = the frames written before the padding.
 *                 FWGPU_ERR_QUEUE_FULL while that much space is not free yet.  After `end`, write and end are refused — with one
 *                 exception: a stream ended BEFORE it was bound sends its end behind the binding, and if fwgpu_sampler_set_sample
 *                 returns FWGPU_ERR_QUEUE_FULL for such a stream the binding stands and only the end was not sent: call end again
 *                 (after a process call) and it is delivered.  An end that reaches the sampler when every frame has been played
 *                 already finishes it there: the blocks in between were starved, and no block of padding is rendered.
 *   status        the counts as of the last completed process call that published them; never blocks.  *written: frames of data
 *                 accepted so far (the padding not counted), *consumed = C, *starved_blocks = U, *finished: the sampler has played past
 *                 the end, or has let go of the stream (another sample set on it, the node removed, the stream destroyed).
 * Binding: fwgpu_sampler_set_sample with a stream id binds it — once, to one sampler (a second binding is FWGPU_ERR_INVALID; bind with
 * at_block 0: the sampler hears of writes only once it holds the stream).  A FIR or resampler node built on a stream id is refused.
 * Setting another sample on the sampler, or removing the node, leaves the stream finished.  fwgpu_sampler_set_playhead_secs and
 * fwgpu_sampler_set_loop_range are refused on a sampler whose sample, as last sent, is a stream: there is no position to seek to and no
 * range to loop.  At most 64 samplers hold a stream at one time.
 * The sampler, at a block of n frames behind the block's messages, with W (frames written that it has been told of), C (consumed), E
 * (the end, or none) and U (starved blocks), all integers:
 *   1. it is a looping sampler over the whole ring, whatever its loop fields said: loop = [0, R), playhead = C mod R.
 *   2. starved: if it is playing and W - C < n then U += 1 and the block is rendered exactly as a block of the same sampler with
 *      playing == 0 — output, silence flags, a smoother and an envelope that do not move; `playing` itself stays 1, nothing else changes.
 *   3. otherwise the block is the looping sampler's block, and C moves by n in exactly the blocks in which that sampler's playhead moves
 *      (a muted voice holds C as it holds its playhead).
 *   4. the end: behind a block that moved C, if E is set and C >= E the sampler does what fwgpu_sampler_pause at the next block's first
 *      frame would do (playing = 0, the envelope to rest) and is finished; fwgpu_sampler_play on a finished stream is ignored.  The block
 *      the end falls into is rendered as a one-shot's last block (frames behind the end are 0.0), so for the blocks that hold data the
 *      output equals that of a one-shot holding the same data, bit for bit — except where the ring's wrap falls in front of the end
 *      inside that same block: those frames are read from the padding (0.0 for the signed and float formats, 1.5e-5 for the unsigned).
 *   5. transport: play and pause are what they are; stop (and a fade's FWGPU_FADE_STOP) acts as pause — a stream does not rewind;
 *      set-playhead and set-loop messages that reach the device anyway are ignored.
 * A voice that holds a stream is never steady: its calls run the control kernel, it leaves no lazy record, the level executor never
 * freezes it, and while any sampler holds a stream one-block callbacks take the per-callback launch instead of the resident realtime
 * kernel.  All of that comes back once the stream is finished (fwgpu_lazy_stats, fwgpu_rt_resident_stats; the resident kernel after
 * the control side has seen `finished`: any write / end / status call looks).  Once per process call the NodeStates of the samplers that
 * hold a stream are copied to pinned memory by one launch, however many there are.  Before it reuses one of its two banks a process
 * call waits for that bank's copy of two calls back: with synchronous calls or paced callbacks that has long completed, but it is a
 * driver call on the audio path that can block, and while a stream is bound it lets fwgpu_process_blocks_device and its kin run at
 * most two calls ahead of the device.  While a stream is bound no call takes the control-ahead mode either: the counts a call publishes
 * are those of frames its kernels have read. */
#define FWGPU_STREAM_RING_FRAMES_MAX 1073741824ull
#define FWGPU_STREAM_RING_MIN_BLOCKS 4
int fwgpu_sample_create_stream(fwgpu_ctx* ctx, int format, uint32_t channels, uint64_t ring_frames); /* -> sample id */
int fwgpu_sample_stream_write(fwgpu_ctx* ctx, int sample, const void* data, uint64_t frames);        /* -> frames accepted, 0..frames */
int fwgpu_sample_stream_write_device(fwgpu_ctx* ctx, int sample, const void* device_data, uint64_t frames);
int fwgpu_sample_stream_end(fwgpu_ctx* ctx, int sample);
int fwgpu_sample_stream_status(fwgpu_ctx* ctx, int sample, uint64_t* written, uint64_t* consumed, uint64_t* starved_blocks, int* finished);

/* ---- processing */
/* FirewheelProcessor::process_interleaved (graph/processor.rs:61-165): host buffers, splits `frames`
 * into max_block_frames blocks, returns after the output has landed in `output`. */
int fwgpu_process_interleaved(fwgpu_ctx* ctx, const float* input, float* output, uint32_t num_in_channels,
                              uint32_t num_out_channels, uint64_t frames, double stream_time_secs,
                              uint32_t stream_status);
/* The same call split in two, for hosts that render ahead (a bounce, an offline render) and keep the host-buffer boundary: `begin` is
 * process_interleaved up to its last launch — the graph-output kernel writes the interleaved frames straight into one of TWO page-locked,
 * device-mapped host staging blocks — and returns a ticket (>= 0); `end` waits for that ticket's last launch and hands the frames to
 * `output`.  With begin(n + 1) called before end(n) the host's share of call n (the wait, the memcpy) overlaps the rendering of call
 * n + 1 and no copy engine or blit kernel sits between two renders: config 2 runs at 0.90 of the device-resident rate this way, 0.84
 * through the synchronous call.  At most two calls in flight; tickets are ended in order.  `end` on the oldest
 * ticket in flight fills `output` on every return (zeros when the device failed, core/node.rs:41-42); `end` on anything else — not a
 * ticket, not the oldest one, a null `output` for a ticket with frames — returns FWGPU_ERR_INVALID, touches nothing (it does not know
 * a size to fill) and leaves the tickets in flight as they were.  `cancel` abandons every ticket in flight up to and including
 * `ticket`: waits for their launches, releases their slots, copies nothing — for hosts that unwind.  Stream INPUTS (`input` non-null)
 * are copied host-to-device by `begin` itself on the ctx stream, behind the previous ticket's render: from pageable memory that copy
 * is synchronous to the host, so a graph with stream inputs gets the output-side overlap only (hand device-resident inputs to
 * fwgpu_process_blocks_device_io for the rest).  Audio-side calls, like process_interleaved itself. */
int64_t fwgpu_process_interleaved_begin(fwgpu_ctx* ctx, const float* input, uint32_t num_in_channels, uint32_t num_out_channels,
                                        uint64_t frames, double stream_time_secs, uint32_t stream_status);
int fwgpu_process_interleaved_end(fwgpu_ctx* ctx, int64_t ticket, float* output);
int fwgpu_process_interleaved_cancel(fwgpu_ctx* ctx, int64_t ticket);
/* Throughput form of the same call: `num_blocks` full blocks, interleaved output written to DEVICE memory
 * `d_output` [num_blocks*max_block_frames*num_out_channels] on the ctx stream, asynchronously (no host
 * sync).  Graph inputs read zeros (fwgpu_process_blocks_device_io takes them from device memory). */
int fwgpu_process_blocks_device(fwgpu_ctx* ctx, uint32_t num_blocks, float* d_output,
                                uint32_t num_out_channels);
/* The same call, also reporting the silence mask read_graph_outputs sees (graph/graph/compiler/schedule.rs:255-287) for every
 * block: d_silence[block * num_out_channels + c] = 1 when graph-output channel c was flagged silent for that block, else 0
 * (device memory, num_blocks * num_out_channels bytes; may be NULL).  These are the flags a shard's partial mix bus carries
 * into the top-level SumNode of a voice-sharded graph (below). */
int fwgpu_process_blocks_device_flags(fwgpu_ctx* ctx, uint32_t num_blocks, float* d_output, uint32_t num_out_channels,
                                      uint8_t* d_silence);
/* ... for graphs WITH stream inputs (an effects rack, a send bus fed from outside): `d_input` = num_blocks * max_block_frames *
 * num_in_channels interleaved frames in DEVICE memory, read on the ctx stream (prepare_graph_inputs + deinterleave,
 * schedule.rs:213-253, util.rs:44-87: channels beyond num_graph_inputs are ignored, missing ones read zeros); NULL / 0 channels = no
 * input.  Asynchronous like the two calls above; the caller keeps `d_input` alive until the stream has passed it. */
int fwgpu_process_blocks_device_io(fwgpu_ctx* ctx, uint32_t num_blocks, const float* d_input, uint32_t num_in_channels, float* d_output,
                                   uint32_t num_out_channels, uint8_t* d_silence);

/* ---- multi-GPU mix bus.  Voices shard across ranks with no exchange until the mix bus; the one exchange step
 * is the top-level SumNode over the R partial buses (nodes/sum.rs:41-136: all inputs silent -> cleared; 2 / 3 / 4 ports ->
 * in1 + in2 (+ in3 (+ in4)); any other count -> out = in0; out += in_p skipping SILENT ports; port = rank order). */
/* That node as one kernel on the ctx stream: d_parts[r] = rank r's interleaved bus of `n_floats` floats in memory this
 * device can read (its own, peer-mapped over xGMI, or the slots of an all-gather), 16-byte aligned; d_out may alias
 * d_parts[0].  Every rank that runs it over the same parts ends up with the bits of the single-process graph (an all-reduce
 * does not: ring order re-associates the f32 sum for R > 2).  Asynchronous; R <= 64.  This form treats no port as silent. */
int fwgpu_bus_sum_ordered(fwgpu_ctx* ctx, const float* const* d_parts, uint32_t n_parts, float* d_out, uint64_t n_floats);
/* ... with the ports' silence flags (sum.rs:52-56,122-124): d_silence[r] = rank r's flags as fwgpu_process_blocks_device_flags
 * wrote them ([blocks][n_channels], or NULL = never silent); the buses are [block][frames_per_block][n_channels] interleaved.
 * d_out_silence (may be NULL) receives the node's out-mask per (block, channel). */
int fwgpu_bus_sum_ordered_flags(fwgpu_ctx* ctx, const float* const* d_parts, const uint8_t* const* d_silence, uint32_t n_parts,
                                float* d_out, uint8_t* d_out_silence, uint64_t n_floats, uint32_t frames_per_block,
                                uint32_t n_channels);
/* The exchange itself, for a host without torch / RCCL (SURVEY §8e path 2: one-shot all-to-all over peer-mapped slots — xGMI
 * is point-to-point, every GPU of a node has a direct link to every other, so each rank STORES its partial bus into its slot
 * on every rank and then each rank adds the R slots it holds in rank order: one link hop instead of the 2(R-1) steps of a
 * ring, and bit-identical to the single-process graph on every rank).
 *   open     (control side) one region of fine-grained HBM on the ctx's device: R slots of max_floats floats + max_silence_bytes
 *            flags, twice (step parity), and R arrival words.  Every rank of an exchange passes the same world and sizes.
 *   export   this rank's FWGPU_EXCHANGE_HANDLE_BYTES-byte handle; the host carries it to the peers by whatever channel it
 *            has (a file, a pipe, MPI_Allgather, torch.distributed.all_gather_object ...).
 *   connect  map a peer's region from its handle: by pointer when the peer lives in this process (virtual shards, several
 *            devices under one host thread: hipDeviceEnablePeerAccess), else hipIpcOpenMemHandle (dmabuf).
 *   push     (audio side, asynchronous on the ctx stream) store d_partial / d_silence into slot `rank` of every region,
 *            release at system scope, raise this rank's arrival word everywhere.
 *   reduce   (audio side, asynchronous) wait ON THE DEVICE for all R arrival words of this step, then the SumNode above
 *            over the R slots -> d_out (+ d_out_silence).  The wait is bounded (set_timeout_ms, default 3000): a peer that
 *            never arrives leaves a ZERO bus and an error fwgpu_bus_exchange_status reports — never a hung device.
 *   step     = push + reduce.  A step of rank g needs every rank's push of the same step: all ranks call step the same
 *            number of times; push and reduce of one exchange must stay on its ctx's stream, in that order (two data
 *            parities make push(s+1) safe while peers still read step s).
 * A reduce with have_silence = 0 treats no port as silent. */
#define FWGPU_EXCHANGE_HANDLE_BYTES 128
typedef struct fwgpu_bus_exchange fwgpu_bus_exchange;
fwgpu_bus_exchange* fwgpu_bus_exchange_open(fwgpu_ctx* ctx, uint32_t rank, uint32_t world, uint64_t max_floats,
                                            uint32_t max_silence_bytes); /* NULL on error: fwgpu_last_error(ctx) */
void fwgpu_bus_exchange_close(fwgpu_bus_exchange* ex);
int fwgpu_bus_exchange_export(fwgpu_bus_exchange* ex, void* handle);
int fwgpu_bus_exchange_connect(fwgpu_bus_exchange* ex, uint32_t peer_rank, const void* handle);
int fwgpu_bus_exchange_set_timeout_ms(fwgpu_bus_exchange* ex, uint32_t ms);
int fwgpu_bus_exchange_push(fwgpu_bus_exchange* ex, const float* d_partial, const uint8_t* d_silence, uint64_t n_floats,
                            uint32_t n_blocks, uint32_t n_channels);
int fwgpu_bus_exchange_reduce(fwgpu_bus_exchange* ex, float* d_out, uint8_t* d_out_silence, uint64_t n_floats, uint32_t n_blocks,
                              uint32_t frames_per_block, uint32_t n_channels, int have_silence);
int fwgpu_bus_exchange_step(fwgpu_bus_exchange* ex, const float* d_partial, const uint8_t* d_silence, float* d_out,
                            uint8_t* d_out_silence, uint64_t n_floats, uint32_t n_blocks, uint32_t frames_per_block,
                            uint32_t n_channels);
/* control side: waits for the ctx stream, then *steps = reduces issued so far, *failed_step = 0 or the first step whose wait
 * ran out of time (then the return value is FWGPU_ERR_DEVICE). */
int fwgpu_bus_exchange_status(fwgpu_bus_exchange* ex, uint64_t* steps, uint64_t* failed_step);
/* control side: waits for the ctx stream; max_wait_us[p] = the longest any reduce so far sat waiting for rank p's arrival, in
 * microseconds (how far the ranks run apart: the slowest rank reads ~0 for everybody, the others read their lead over it).
 * Returns the world size; reset != 0 clears the maxima. */
int fwgpu_bus_exchange_wait_stats(fwgpu_bus_exchange* ex, uint64_t* max_wait_us, uint32_t cap, int reset);
/* ---- the mix bus over RCCL (north_star: "a single RCCL all-reduce over xGMI for the final mix bus"; the node being computed is the
 * top-level R-port SumNode, nodes/sum.rs:111-133).  librccl is dlopen'ed by the first of these calls, never linked: a host that does
 * not shard does not load it.  One process per GPU; rank 0 makes the unique id, the host carries its FWGPU_RCCL_UNIQUE_ID_BYTES bytes
 * to every rank (the side channel that carries the exchange's handles), every rank creates its communicator on its ctx's device.
 *   unique_id          rank 0: ncclGetUniqueId.
 *   comm_create        collective (ncclCommInitRank): every rank of the id calls it; NULL on error (fwgpu_last_error of the ctx).
 *                      Control side; the communicator belongs to the ctx and must be destroyed before it.
 *   allreduce_rccl     ncclAllReduce(sum) IN PLACE on the ctx stream, asynchronous.  The ring re-associates the f32 sum for more
 *                      than two ranks: within 1e-6 relative of the single-process graph, not its bits; silence flags play no part
 *                      (a silent shard's bus is cleared zeros, and x + 0 = x).
 *   allgather_ordered  ncclAllGather of the partial buses and of their per-(block, channel) silence flags (as
 *                      fwgpu_process_blocks_device_flags wrote them; NULL = never silent), then fwgpu_bus_sum_ordered_flags over
 *                      the gathered slots: sum.rs's port order and silent-port rule, bit-identical to the single-process graph on
 *                      every rank.  n_floats a multiple of 4; d_out 16-byte aligned, may alias d_bus; d_out_silence may be NULL.
 * Audio-side calls like the process calls they follow (same stream).  fwgpu_rccl_last_error: the text of the last failure of a
 * call that has no ctx to report through (unique_id). */
#define FWGPU_RCCL_UNIQUE_ID_BYTES 128
typedef struct fwgpu_rccl_comm fwgpu_rccl_comm;
int fwgpu_rccl_unique_id(uint8_t* id);
fwgpu_rccl_comm* fwgpu_rccl_comm_create(fwgpu_ctx* ctx, const uint8_t* id, uint32_t world, uint32_t rank);
int fwgpu_rccl_comm_destroy(fwgpu_rccl_comm* comm);
int fwgpu_rccl_comm_info(fwgpu_rccl_comm* comm, uint32_t* world, uint32_t* rank);
int fwgpu_bus_allreduce_rccl(fwgpu_rccl_comm* comm, float* d_bus, uint64_t n_floats);
int fwgpu_bus_allgather_ordered(fwgpu_rccl_comm* comm, const float* d_bus, const uint8_t* d_silence, float* d_out,
                                uint8_t* d_out_silence, uint64_t n_floats, uint32_t frames_per_block, uint32_t n_channels);
const char* fwgpu_rccl_last_error(void);
int fwgpu_synchronize(fwgpu_ctx* ctx);

/* ---- level meter (FWGPU_METER; SPEC, DESIGN.md section 6: the "decibel meter" of the reference's DESIGN_DOC.md:11-28).  The mix lives in
 * HBM and the throughput calls never bring audio to the host: a meter node measures a bus ON the device, one 16-byte record per
 * (block, input channel), and the host fetches only those.  n_in in 1..64; n_out == n_in passes the audio and the silence mask
 * through bit for bit (a channel flagged silent is zero-filled and flagged, its record reads {+0, +0, 0, frames} without touching the
 * buffer), n_out == 0 is a tap that only measures; any other shape — and a ring_blocks outside 1..65536, NaN, a fraction — fails
 * activation at fwgpu_update.  No parameters after creation, no smoother, no messages.
 *   peak         max |x[i]| over the block's `frames` samples, NaN samples ignored (fmaxf); never negative.
 *   over         samples with |x[i]| > 1.0f (NaN does not count).
 *   sum_squares  f32, no FMA, in this fixed order: 256 accumulators acc[j] = +0.0, acc[i % 256] += x[i] * x[i] for i ascending;
 *                t[l] = ((acc[4l] + acc[4l+1]) + acc[4l+2]) + acc[4l+3] for l in 0..63; then t[l] += t[l + h] for l < h with
 *                h = 32, 16, 8, 4, 2, 1; the result is t[0].  (The order is part of the numeric SPEC.)
 *   frames       the block's length: max_block_frames, or less for the short last block of a fwgpu_process_interleaved call.
 * The ctx counts every block it processes, full or partial, over every process call; block g's records sit in slot g % ring_blocks of
 * the node's ring, which is zeroed at activation and travels across plan changes like every node state.  One launch covering more
 * blocks than the ring holds writes only its last ring_blocks.  A 2 -> 2 meter in the master chain (between the root SumNode and
 * graph_out) leaves the fused plan kind and its lazy calls as they are: it is one more launch per batch; a master chain of any kind
 * takes one-block calls off the one-launch / resident realtime paths (fwgpu_rt_path_stats paths[2]).  Anywhere else — a leaf bus, a
 * voice chain, a tap — the level executor renders the meter and the fused plans keep what they can.  Blocks run through
 * fwgpu_node_process are NOT recorded (that call passes the audio and the mask through and returns). */
typedef struct fwgpu_meter_reading {
    float peak;
    float sum_squares;
    uint32_t over;
    uint32_t frames;
} fwgpu_meter_reading;
/* Audio-side call, like fwgpu_synchronize: waits for the ctx stream, stores the ctx's block count in *blocks_done (when non-NULL, on
 * every return that has a valid ctx), copies the records of blocks [first_block, first_block + n) to out[i * n_in + c] and returns n
 * <= num_blocks: how many of those blocks exist yet.  num_blocks == 0 (out may be NULL) only reports the count.  FWGPU_ERR_INVALID:
 * `node` is not a meter of the installed plan; first_block + ring_blocks < *blocks_done (older than the ring retains); first_block is
 * older than the first block the meter was part of a plan for; out == NULL with blocks requested.  Polling from a control thread
 * without a stream wait is out of scope (it would need a pinned, device-mapped ring). */
int64_t fwgpu_meter_read(fwgpu_ctx* ctx, int64_t node, uint64_t first_block, uint32_t num_blocks, fwgpu_meter_reading* out,
                         uint64_t* blocks_done);

/* ---- spectrum meter (SPEC): WHERE in frequency the energy of a bus is — what a spectrum display, a beat or onset
 * detector or an audio-reactive effect reads — measured on the device like the levels.  A FWGPU_METER created with two or more
 * parameters, `ring_blocks, fft_size, bands`, is a spectrum meter; created with none or one it is the plain node above.  fft_size N is
 * one of 256, 512, 1024, 2048, 4096; bands is a whole number in 0..N/2 (default 32 when only two parameters are given); n_in in 1..8,
 * n_out == n_in or 0.  NaN, Inf, a fraction, another N, bands > N/2, n_in > 8 and ring_blocks * n_in * B > 2^24 floats (B: the floats
 * of one record, below) fail activation at fwgpu_update.  The level records, the audio and the silence flags are exactly a plain
 * meter's, fwgpu_meter_read included.  Besides them the node keeps one record of B floats per (block, input channel), block g in slot
 * g % ring_blocks of a second ring with the rules of the first.  Per input channel, x[n] the frames since the node's activation (every
 * frame of every block, full or short; x[n < 0] = +0.0; a block flagged silent counts as +0.0 and is not read), for block g with last
 * frame n_g, all in f32, every operation rounded, no FMA:
 *   window    v[i] = x[n_g - N + 1 + i] * w[i], i in 0..N-1, w[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / N)) (periodic Hann, host, f64)
 *   transform complex radix-2 decimation-in-time FFT of (v, 0); twiddles wr[k] = (float)cos(2.0 * M_PI * k / N), wi[k] =
 *             (float)(-sin(2.0 * M_PI * k / N)), k < N/2 (host tables); input in bit-reversed order, re[i] = v[bitrev(i)], im[i] = +0.0;
 *             stages h = 1, 2, 4, .., N/2: for every group of 2h consecutive elements and j < h, a = element j, b = element j + h,
 *             k = j * (N / (2h)):  tr = (wr[k]*b.re) - (wi[k]*b.im), ti = (wr[k]*b.im) + (wi[k]*b.re),
 *             a' = (a.re + tr, a.im + ti), b' = (a.re - tr, a.im - ti)
 *   power     P[k] = ((re[k]*re[k]) + (im[k]*im[k])) * (16.0f / (N*N)), k in 0..N/2: a full-scale sine on a bin centre reads 1.0 at its
 *             bin and 0.25 at each neighbour
 *   bands     band b = ((P[e[b]] + P[e[b]+1]) + ...) + P[e[b+1]-1], one ascending chain of f32 adds.  bands == 0: B = N/2 + 1, e[b] = b
 *             (every bin, DC included).  Otherwise B = bands, M = N/2, e[0] = 1, e[B] = M + 1 and for 0 < b < B
 *             e[b] = max(e[b-1] + 1, min(M + 1 - (B - b), (int)floor(pow((double)M, (double)b / B) + 0.5))): strictly increasing
 * The hop is the block: windows overlap when the block is shorter than N; when it is longer only its last N frames are seen.  Blocks
 * run through fwgpu_node_process pass the audio, are not recorded and leave the window's history untouched.  No parameters after
 * creation. */
#define FWGPU_SPECTRUM_FFT_MIN 256
#define FWGPU_SPECTRUM_FFT_MAX 4096
#define FWGPU_SPECTRUM_CH_MAX 8
#define FWGPU_SPECTRUM_BANDS_DEFAULT 32
/* fwgpu_meter_read's contract and error cases for the spectrum records: out[(i * n_in + c) * B + b].  FWGPU_ERR_INVALID also for a plain
 * meter. */
int64_t fwgpu_spectrum_read(fwgpu_ctx* ctx, int64_t node, uint64_t first_block, uint32_t num_blocks, float* out, uint64_t* blocks_done);
/* Audio-side call.  Returns B, the floats of one record of spectrum meter `node` of the installed plan (FWGPU_ERR_INVALID: not one);
 * stores N and the `bands` parameter (when non-NULL) and up to edges_cap of the B + 1 edges: band b covers bins e[b] .. e[b+1] - 1,
 * bin k is centred on k * sample_rate / N Hz. */
int fwgpu_spectrum_layout(fwgpu_ctx* ctx, int64_t node, uint32_t* fft_size, uint32_t* bands, uint32_t* edges, uint32_t edges_cap);

/* ---- look-ahead limiter (FWGPU_LIMITER; SPEC).  The remedy that goes with the meter's `over` count and, like it,
 * leaves the mix in HBM: a linked-channel brickwall limiter with a hold, written as FIR stages — a sliding minimum of the target gain and
 * a 64-term moving average in a fixed order of summation — so it has no recurrence in time, its K blocks of a batch render in parallel,
 * and its output is bit-exact against a dozen lines of numpy (tests/test_limiter.py).  n_in == n_out in 1..8, refused at fwgpu_add_node
 * otherwise; a ceiling that is NaN, infinite or outside 0.001..1000 and a hold_frames that is NaN, a fraction or outside 0..1920 fail
 * activation at fwgpu_update (FWGPU_ERR_INVALID).  No parameters after creation (fwgpu_node_set_param is refused), no smoother, no
 * messages.  With C = ceiling, H = hold_frames, x_c[n] input channel c at frame n since the node's activation (every frame of every
 * block, full or short; +0.0 for n < 0; a channel flagged silent for a block counts as +0.0):
 *   key[n] = max over c of |x_c[n]|      (fmaxf: a NaN sample is ignored; never negative)
 *   t[n]   = key[n] > C ? C / key[n] : 1.0f                      (IEEE f32 division)
 *   m[n]   = min of t[k], k in [n-63-H, n], t[k < 0] = 1.0f
 *   s[n]   = (((m[n-63] + m[n-62]) + m[n-61]) + ...) + m[n]      (64 terms, one ascending chain of f32 adds, no FMA)
 *   y_c[n] = x_c[n-63] * (s[n] * 0.015625f)
 * The output is late by FWGPU_LIMITER_LATENCY frames.  |y| <= C * (1 + 66 * 2^-24): every m[j], j in [n-63, n], has frame n-63 in its
 * window.  While nothing exceeds C the gain is exactly 1.0f and the output is the delayed input bit for bit; after an over the gain holds
 * for H + 64 frames and returns along a 64-frame staircase average — a safety limiter, not a mastering one.  Outputs are never flagged
 * silent.  The node's state is the last H + 128 input frames per channel, zeroed at activation and kept across plan changes.  A 2 -> 2
 * limiter in the master chain leaves the fused plan kind and its lazy calls as they are: one more launch per batch, as a meter; anywhere
 * else the level executor renders it.  fwgpu_node_process renders it block by block with the history kept between calls. */
#define FWGPU_LIMITER_LATENCY 63

/* ---- sidechain ducker (FWGPU_DUCKER; SPEC).  A key bus turns another bus down — dialogue over music — without
 * either leaving HBM: the first node with a sidechain, an input that steers the node and is not heard.  n_out = n outputs and
 * n_in = n + k inputs, n and k in 1..8: inputs 0..n-1 are the main bus, inputs n..n+k-1 the key; any other shape is refused at
 * fwgpu_add_node.  A threshold that is NaN, infinite or outside 1e-6..1000, a depth outside 0..1, an attack_frames or release_frames
 * that is NaN, a fraction or outside 1..32768 and a hold_frames that is NaN, a fraction or outside 0..32768 fail activation at
 * fwgpu_update (FWGPU_ERR_INVALID).  No parameters after creation (fwgpu_node_set_param is refused), no smoother, no messages.  With
 * T = threshold, D = depth, A, R, H = attack, release and hold frames, x_c[n] main channel c and k_j[n] key channel j at frame n since
 * the node's activation (every frame of every block, full or short; everything false or zero for n < 0; a key channel flagged silent
 * for a block counts as +0.0 and is not read):
 *   key[n]  = max over j of |k_j[n]|      (fmaxf from +0.0: a NaN sample is ignored; never negative)
 *   on[n]   = key[n] > T                  (a sample of exactly T does not open the gate)
 *   open[n] = on[k] for some k in [n-H, n]
 *   ca[n]   = number of k in (n-A, n] with open[k]        cr[n] = number of k in (n-R, n] with open[k]        (integers)
 *   a[n]    = (float)ca[n] / (float)A     r[n] = (float)cr[n] / (float)R                (IEEE f32 division, correctly rounded)
 *   u[n]    = fmaxf(a[n], r[n])           (the ducking amount, 0..1)
 *   g[n]    = 1.0f - ((1.0f - D) * u[n])  (1.0f - D once; one product, one subtraction, no FMA)
 *   y_c[n]  = x_c[n] * g[n]
 * No latency.  No recurrence in time: the gain is a function of integer counts over windows of the key, so the K blocks of a batch
 * render in parallel and the output is bit-exact against a few lines of numpy (tests/test_ducker.py) in any order of evaluation.
 * While the gate has been closed for max(A, R) + H frames g is exactly 1.0f and the output is the input bit for bit; after max(A, R)
 * open frames g = 1.0f - (1.0f - D); u never steps by more than 1 / min(A, R).  With A <= R the gain falls over A frames and comes
 * back linearly over R.  An open run shorter than R ducks to full depth in A frames, recovers over A frames to the plateau len / R
 * and leaves over the rest of R: the price of having no recurrence.  A main channel flagged silent gives an output that is
 * zero-filled and flagged; any other output is never flagged.  The node's state is the last max(A, R) + H gate bits on[], bit-packed,
 * zeroed at activation (the gate was closed) and kept across plan changes.  A ducker is never part of a fused plan's master chain
 * (it is not 2 -> 2): the level executor renders it.  fwgpu_node_process renders it block by block with the history kept between
 * calls. */

/* ---- bus compressor (FWGPU_COMPRESSOR; SPEC).  The third dynamics tool of a bus, beside the limiter and the
 * ducker: it holds an SFX or dialogue bus together, and on the master in front of the limiter it leaves the limiter little to do.
 * Self-keyed with linked channels: n_in == n_out = n in 1..FWGPU_COMPRESSOR_CH_MAX, any other shape is refused at fwgpu_add_node (a
 * keyed bus is the ducker's job).  A threshold T that is NaN, infinite or outside 1e-6..1000, a ratio outside 1..1000, a knee_db outside
 * 0..24, an attack_frames A or release_frames R that is NaN, a fraction or outside 1..FWGPU_COMPRESSOR_WIN_MAX, a hold_frames H that is
 * NaN, a fraction or outside 0..FWGPU_COMPRESSOR_HOLD_MAX and a makeup M outside 0.001..1000 fail activation at fwgpu_update
 * (FWGPU_ERR_INVALID).  No parameters after creation (fwgpu_node_set_param is refused), no smoother, no messages, no latency.
 * At activation, in f64 with the host's libm:
 *   T0   = (float)(T * 10^(-knee_db / 40))                      (the level at which the knee begins)
 *   G[i] for i in 0..320, 16 knots per octave over 20 octaves: knot i sits at u_i = 2^(i / 16) * (1 + (i % 16) / 16) (i / 16 the integer
 *          quotient); with over = 20 * log10(u_i) - knee_db / 2 and slope = 1 / ratio - 1:
 *          gr = slope * (over + knee_db / 2)^2 / (2 * knee_db)   if knee_db > 0 and 2 * |over| <= knee_db
 *          gr = slope * over                                     otherwise, if over > 0;      gr = 0 otherwise
 *          G[i] = (float)10^(gr / 20)                            (G[0] is exactly 1.0f and G never rises)
 * With x_c[n] channel c at frame n since the node's activation (every frame of every block, full or short; a channel flagged silent
 * for a block counts as +0.0 and is not read):
 *   key[n] = max over c of |x_c[n]|         (fmaxf from +0.0: a NaN sample is ignored; never negative)
 *   u[n]   = key[n] / T0                    (IEEE f32 division)
 *   t[n]   = 1.0f                           if !(u[n] > 1.0f); else with d = bits(u[n]) - 0x3F800000, i = d >> 19,
 *                                           fr = (float)(d & 0x7FFFF) * 2^-19 (exact):
 *            G[320]                         if i >= 320 (an infinite key included)
 *            G[i] + ((G[i+1] - G[i]) * fr)  otherwise (every operation a separately rounded f32 operation, no FMA)
 *   q[n]   = (uint32)((t[n] * 65535.0f) + 0.5f)            (0..65535; q[n < 0] = 65535: unity)
 *   m[n]   = min of q[k], k in [n-H, n]                     (the hold: a peak detector over H frames)
 *   ca[n]  = sum of m[k], k in (n-A, n]     cr[n] = sum of m[k], k in (n-R, n]              (exact integers, below 2^32)
 *   a[n]   = (float)ca[n] / (float)(A * 65535)              r[n] = (float)cr[n] / (float)(R * 65535)
 *   g[n]   = fminf(a[n], r[n])
 *   y_c[n] = x_c[n] * (g[n] * M)            (g * M one product, then one product per channel)
 * No recurrence in time: the gain is a function of integer sums over windows of q, so the K blocks of a batch render in parallel and
 * the output is bit-exact against a few lines of numpy (tests/compressor_model.py) in any order of evaluation.  While the level has
 * stayed at or below T0 for max(A, R) + H frames g is exactly 1.0f, and with M = 1 the output is the input bit for bit.  g never
 * exceeds 1 and never falls below G[320] minus the 1/65535 quantum.  With A <= R a step up in level takes the gain down linearly over A
 * frames; a step down lets it back linearly over R, which begins H frames later.  A burst shorter than R reaches full reduction in A
 * frames, returns over A to the plateau 1 - (1 - t) * len / R and leaves over the rest of R: the price of having no recurrence, as
 * for the ducker.  A steady level settles at q / 65535, within 2^-16 of the curve; the table's interpolation stays within 0.01 dB of
 * the exact curve.  ratio == 1 is the identity times M.  A channel flagged silent gives an output that is zero-filled and flagged and
 * still lets the others drive the gain; nothing else is flagged.  The node's state is the table and the last max(A, R) + H values of
 * q as 16-bit words, unity at activation and kept across plan changes.  A 2 -> 2 compressor may sit in a fused plan's master chain, as
 * a limiter may: one more launch per batch, the plan stays.  fwgpu_node_process renders it block by block with the history kept
 * between calls. */
#define FWGPU_COMPRESSOR_WIN_MAX 32768
#define FWGPU_COMPRESSOR_HOLD_MAX 2048
#define FWGPU_COMPRESSOR_CH_MAX 8

/* ---- latency compensation (FWGPU_DELAY_COMP and the latency queries; SPEC).  A limiter makes its bus
 * FWGPU_LIMITER_LATENCY frames late; summed with a bus that is not, the two are misaligned, and a dry signal mixed with its limited
 * copy comb-filters.  FWGPU_DELAY_COMP is the remedy: a pure delay of D = `frames` whole frames, n_in == n_out in 1..8, refused at
 * fwgpu_add_node otherwise.  A `frames` that is NaN, a fraction or outside 0..FWGPU_DELAY_COMP_MAX fails activation at fwgpu_update
 * (FWGPU_ERR_INVALID).  No parameters after creation (fwgpu_node_set_param is refused), no smoother, no messages.  With x_c[n] input
 * channel c at frame n since the node's activation (every frame of every block, full or short; +0.0 for n < 0; a channel flagged
 * silent for a block counts as +0.0 for that block and is not read):
 *   y_c[n] = x_c[n - D]
 * a copy, with no arithmetic: -0.0, infinities, subnormals and NaN payloads come out with the bits they went in with; D = 0 is the
 * identity.  (FWGPU_DELAY is an effect: its time is in seconds, it has no D = 0, and its output (x * dry) + (d * mix) is arithmetic.)
 * Silence flags, which downstream sums rely on: per channel one integer loud_c, 0 at activation.  Output channel c of a block of F
 * frames is zero-filled and flagged if and only if its input is flagged for this block and loud_c == 0 in front of the block;
 * otherwise it is written and not flagged.  Behind the block loud_c = D if the input was not flagged, max(0, loud_c - F) otherwise.
 * So an output block is flagged exactly when the D frames in front of it and the block itself were all flagged or lie before the
 * activation.  The node's state is the last D input frames per channel (flagged blocks enter as zeros) and the counters, zeroed at
 * activation and kept across plan changes.  No recurrence in time: every block of a batch renders in parallel, whatever D and the block
 * length are.  The level executor renders the node (a kernel of its own, k_delay_comp); the fused plans around it keep what they can.
 * fwgpu_node_process renders it block by block with the history kept between calls. */
#define FWGPU_DELAY_COMP_MAX 8192
/* The latency queries are pure host code over the CURRENT edge set: no fwgpu_update is needed first.
 *   own(v)    = FWGPU_LIMITER_LATENCY for a limiter, `frames` for a FWGPU_DELAY_COMP node, 0 for every other kind (FWGPU_DELAY included:
 *               an effect, not latency)
 *   in(v, p)  = out(source of input port p), for a connected port
 *   out(v)    = own(v) + max over v's connected input ports p of in(v, p)       (a node without connected inputs: own(v))
 * fwgpu_node_latency: own(node) into *frames; FWGPU_ERR_INVALID for an unknown node. */
int fwgpu_node_latency(fwgpu_ctx* ctx, int64_t node, uint32_t* frames);
/* one connected input port that the other inputs of its node are later than: delaying this edge by lead_frames aligns it */
typedef struct fwgpu_latency_skew {
    int64_t node;         /* the node the edge arrives at */
    uint32_t port;        /* its input port */
    uint32_t lead_frames; /* max over the node's connected ports q of in(node, q), minus in(node, port): > 0 */
} fwgpu_latency_skew;
/* Every connected input (v, p) with lead = max_q in(v, q) - in(v, p) > 0, a sidechain's inputs and graph_out's included, in ascending
 * order of the node's slot (the low 32 bits of its id), then of the port.  Returns the total count and writes at most `cap` records
 * (`out` may be NULL with cap 0).  One pass, O(nodes + edges).  A cyclic edge set (fwgpu_connect with check_for_cycles = 0) returns
 * the error fwgpu_update would return, FWGPU_ERR_COMPILE_CYCLE.  A FWGPU_DELAY_COMP node of lead_frames on each reported edge leaves
 * every out(v) as it was — the delayed edge now arrives when the node's latest input does — and the report empty: one pass of
 * compensation is enough (FirewheelGpuCtx.compensate_latency does exactly that). */
int64_t fwgpu_graph_latency_report(fwgpu_ctx* ctx, fwgpu_latency_skew* out, uint32_t cap);
/* the arrival latency at the graph output node, max over its connected ports (0 with none): what picture sync needs */
int fwgpu_graph_output_latency(fwgpu_ctx* ctx, uint32_t* frames);

/* ---- crossfader (FWGPU_CROSSFADE; SPEC).  Two buses blended along an automated curve: explore music into
 * combat music over three seconds with an ease, one room's reverb return into another's, a fade to black — one message instead of
 * one fwgpu_node_set_param per block.  n_out = n outputs and n_in = 2n inputs, n in 1..8: inputs 0..n-1 are bus A, inputs n..2n-1
 * bus B; any other shape is refused at fwgpu_add_node.  With bus B left unconnected the node is a fader of bus A with the same
 * curves.  Creation parameters: position (0 = all A, 1 = all B) and law; a position that is NaN or outside 0..1 and a law other than
 * 0 or 1 fail activation at fwgpu_update (FWGPU_ERR_INVALID).  The state is the node time T — a 64-bit count of the frames rendered
 * since activation, full and short blocks alike —, one segment {P0, P1, t0, dur, shape, x1, y1, x2, y2} and the law; dur == 0 means
 * at rest at P1.  No smoother, no ext slice; kept across plan changes.  Every operation below is a separately rounded f32 operation,
 * no FMA.  The position of frame n (node time), with k = n - t0:
 *   dur == 0 or k >= dur:  p = P1
 *   otherwise              u = (float)k / (float)dur                  (IEEE division; both conversions exact, dur <= 2^24)
 *     shape 0 (linear):    y = u
 *     shape 1 (cubic Bezier easing through (0,0), (x1,y1), (x2,y2), (1,1)):  y = 0 when u == 0, otherwise with
 *                          c = 3*a; b = 3*(d - a) - c; q = (1 - c) - b;  B(t; a, d) = ((q*t + b)*t + c)*t:
 *                            lo = 0, hi = 1;  24 times: m = (lo + hi) * 0.5f; if B(m; x1, x2) < u then lo = m else hi = m
 *                            t = (lo + hi) * 0.5f;  y = B(t; y1, y2)
 *     p = P0 + ((P1 - P0) * y), clamped: p = fminf(fmaxf(p, 0), 1)    (a curve may overshoot; the position does not)
 * Gains: linear law a = 1.0f - p, b = p; equal-power law a = sqrtf(1.0f - p), b = sqrtf(p), correctly rounded.  Output:
 *   p == 0:  y_c = A_c, a copy bit for bit        p == 1:  y_c = B_c, a copy bit for bit        otherwise  y_c = (A_c * a) + (B_c * b)
 * An input channel flagged silent for the block (an unconnected input is one) counts as +0.0 and is not read.  A block is at rest
 * when dur == 0 or T - t0 >= dur at its first frame.  Output channel c is zero-filled and flagged exactly when A_c and B_c are both
 * flagged, or the block is at rest at p == 0 and A_c is flagged, or the block is at rest at p == 1 and B_c is flagged; otherwise it is
 * written and not flagged.  Time advances in every case.  No latency.  The position is a pure function of the node time, so the
 * blocks of a batch that carries no message for the node render in parallel; only the batch in which a message lands is walked in
 * order.  The level executor renders the node (inside k_level); the voice banks in front of it keep their fused kernels.
 * fwgpu_node_process renders it block by block with the node time kept between calls.
 *
 * fwgpu_crossfade_to: from the start of block `at_block` of the next process call, move to `position` over `frames` frames along
 * `shape` (0 linear, 1 Bezier with the control values x1, y1, x2, y2; they are ignored by shape 0).  Applied with T the node time of
 * that block's first frame: P0 = the position the rule above gives frame T under the old segment — a retarget in mid-fade starts
 * exactly where the old fade stands —, t0 = T, dur = frames, P1 = position.  frames == 0 is a jump.  Several messages for one block
 * apply in order.  FWGPU_ERR_INVALID for a node of another kind, a position outside 0..1, frames > FWGPU_CROSSFADE_FRAMES_MAX, a
 * shape other than 0 or 1, x1 or x2 outside 0..1, y1 or y2 outside -1..2, and any NaN. */
#define FWGPU_CROSSFADE_FRAMES_MAX 16777216
#define FWGPU_CROSSFADE_CH_MAX 8
int fwgpu_crossfade_to(fwgpu_ctx* ctx, int64_t node, float position, uint32_t frames, int shape, float x1, float y1, float x2, float y2,
                       uint32_t at_block);

/* ---- FIR reverb morph: two impulse responses over one history, blended along the crossfader's curve (SPEC).
 * A FWGPU_FIR node created with ONE parameter is the plain node.  Created with two or more it is morph-capable: slot A and slot B each
 * hold an impulse response, zero-padded to the node's tap capacity T (max_taps, or the longer of the two), and both convolve the SAME
 * input history — one ring per channel, appended every block whatever the position.  The slot sum s_X[n] is bit for bit the output of
 * a plain FIR node whose sample is slot X's impulse response padded to T (window T-1+frames, segments of 4096 positions, one fma
 * chain per segment from +0.0, partials added in order, + (+0.0f)); channel c convolves with channel min(c, C_h - 1); an empty slot's
 * sum is +0.0.  Position p of frame n, node time, the segment, the retarget rule and the gains a, b are the crossfader's above, and
 *   p == 0:  y = s_A, a copy        p == 1:  y = s_B, a copy        otherwise  y = (s_A * a) + (s_B * b)   (no FMA)
 * A block at rest (dur == 0, or the segment over at its first frame) at p == 0 leaves slot B idle — no matrix work —, at p == 1 slot
 * A; in every other block both slots run.  The out flag is cleared as a plain node's; latency is unchanged.  A bad ir_b, max_taps
 * (not 0 and shorter than an impulse response, or above 2^24), position or law is refused by the next fwgpu_update, as a crossfader's.
 *
 * fwgpu_fir_morph: fwgpu_crossfade_to for such a node — same message, same refusals (and FWGPU_ERR_INVALID for a plain FIR node).
 *
 * fwgpu_fir_set_ir: exchange the impulse response of `slot` (0 = A, 1 = B) for `sample` (slot 1: or -1, an empty slot) — a graph
 * edit: it takes effect with the plan the next fwgpu_update builds.  The new impulse response convolves the history the node has: when
 * it fades in, its tail is complete from the first frame.  FWGPU_ERR_INVALID when the node is not morph-capable, the sample is a
 * stream, empty or longer than T, -1 is given for slot 0 (slot A's rows append the history), or the slot is not inaudible: the last
 * morph sent (none: the creation position) must target exactly the OTHER slot's end, and its last frame must lie within the frames of
 * the process calls started so far (a call counts from its start: the edit is adopted by a later call's plan, never by the one in
 * flight).  A morph sent after the edit and before that update — or before the node's first update — is held and released by the
 * update; it starts only then, and while one is held both slots count as audible.  A sample
 * in either slot cannot be destroyed; its converted copy is cached per (sample, channel, T) and freed with its last user.
 *
 * fwgpu_fir_morph_stats: GEMM workgroups of morph groups since the context was created — that ran / that returned because every row of
 * their tile was idle in their block. */
int fwgpu_fir_morph(fwgpu_ctx* ctx, int64_t node, float position, uint32_t frames, int shape, float x1, float y1, float x2, float y2,
                    uint32_t at_block);
int fwgpu_fir_set_ir(fwgpu_ctx* ctx, int64_t node, int slot, int sample);
int fwgpu_fir_morph_stats(fwgpu_ctx* ctx, uint64_t* tiles_run, uint64_t* tiles_skipped);

/* ---- resampling source: a ratio glide (Doppler) in one message (SPEC).
 * fwgpu_resampler_glide: from the first frame of block `at_block` of the next process call, move the node's ratio to `ratio` over
 * `frames` output frames, linearly in the 32.32 step.  With S the step the node has reached there (u64, 32.32), S1 the step param 1
 * would set for `ratio` (clamped to [1/256, 256], rounded half away) and N = frames:
 *   inc = (int64)(S1 - S) / (int64)N   (truncated toward zero; |S1 - S| < 2^40),   left = N,   target = S1
 * Per rendered frame while left > 0: the frame is taken at pos; then pos += step; step += inc; left -= 1; when left reaches 0,
 * step = target exactly.  Closed form for a run of m <= left frames from (pos0, step0), in wrapping u64 arithmetic:
 *   step_i = step0 + i*inc,   pos_i = pos0 + i*step0 + inc * (i*(i-1)/2)
 * Every step_i lies between the two ends, so the position never goes backwards.  Everything else is the resampler as it is: phase
 * (p >> 27) & 31, the 16-tap fmaf chain ascending from +0.0, a loop takes pos %= len << 32 behind each block, a one-shot stops once
 * (pos >> 32) >= len + 8, and a paused or sample-less source renders nothing and advances nothing, the glide included.
 * frames == 0 is exactly param 1 (a step).  Param 1 during a glide ends it and sets the step; a second glide starts from the step the
 * first has reached; a seek (param 4) and pause / play (param 3) leave the glide as it is; several messages for one block apply in
 * send order.  A voice inside a glide is not steady: its calls run the control kernel, and lazy calls resume with the first call
 * behind the glide.  FWGPU_ERR_INVALID for a node of another kind, a NaN ratio, or frames > FWGPU_RESAMPLER_GLIDE_FRAMES_MAX. */
#define FWGPU_RESAMPLER_GLIDE_FRAMES_MAX 16777216
int fwgpu_resampler_glide(fwgpu_ctx* ctx, int64_t node, float ratio, uint32_t frames, uint32_t at_block);

/* ---- volume and pan: a gain ride, param 0 moved along a curve in one message (SPEC).
 * fwgpu_gain_ride: `node` is a FWGPU_VOLUME or a FWGPU_STEREO_PAN node and `value` what its param 0 takes (percent_volume, or pan in
 * -1..1).  From the first frame of block `at_block` of the next process call the node's gain — a volume's one gain, a pan's left and
 * right gain, each on its own — travels from where it stands to the f32 gain(s) param 0 would set for `value` (G1_c), over `frames`
 * frames, along the crossfader's curve (`shape`, x1 .. y2: as fwgpu_crossfade_to takes and validates them).  Per gain c, with G0_c the
 * gain in force at that block's first frame (a ride in flight: its value there; else what the smoother last gave), N = frames and k the
 * frames of the ride rendered so far, the gain of the frame j frames ahead is
 *   ride_c(j) = N == 0 || k + j >= N ? G1_c
 *             : clamp(G0_c + (d_c * y((float)(k + j) / (float)N)), min(G0_c, G1_c), max(G0_c, G1_c)),   d_c = G1_c - G0_c, computed once
 * y(u) = u for shape 0; for shape 1 the crossfader's curve bit for bit (above: y = 0 at u == 0, else 24 bisection steps on
 * B(t; x1, x2) < u, then B(t; y1, y2)).  Every operation is a separately rounded f32 operation, the division IEEE, no FMA.  The clamp
 * replaces the crossfader's clamp to 0..1: an overshooting curve flattens at the ends, the gain never leaves the interval and never
 * goes negative.  The ride happens in the GAINS, per ear for a pan, as a spatialiser move travels: a ride from hard left to hard right
 * therefore dips in power at the middle (each ear passes 0.5 where equal power wants 0.707) — a ride that must hold power is two
 * segments through the centre.  The message puts the smoother(s) at rest at the target(s); in a ride the smoother is not run and the
 * volume's mute test (gain < 1e-5) is not applied; an input flagged silent still gives cleared, flagged outputs.  Behind every block
 * the node is processed in, silent input or not, k += the block's frames; once k >= N the node is at rest, bit for bit a node set to
 * the target whose smoother has settled (a volume that rode to 0 mutes from the next block on).  frames == 0 is a step: the hard set
 * with no 10 ms glide.  A second ride starts where the first stands.  Param 0 during a ride ends it: the smoother(s) are reset to the
 * ride's current value(s), then the parameter is set, so the one-pole glides on from there.  Several messages for one block apply in
 * send order.  A voice with a stage in a ride is not steady: its calls run the control kernel, and lazy calls resume with the first
 * call behind the ride; one-block calls take the launch sequence while a ride may be in flight.  FWGPU_ERR_INVALID for a node of
 * another kind, a NaN or infinite value, frames > FWGPU_GAIN_RIDE_FRAMES_MAX, or a shape or control value fwgpu_crossfade_to refuses. */
#define FWGPU_GAIN_RIDE_FRAMES_MAX 16777216
int fwgpu_gain_ride(fwgpu_ctx* ctx, int64_t node, float value, uint32_t frames, int shape, float x1, float y1, float x2, float y2,
                    uint32_t at_block);

/* ---- spatialiser: a move of the source in one message (SPEC).
 * fwgpu_spatial_move: from the first frame of block `at_block` of the next process call, move the node from where it stands to what
 * params 0..2 would set for (x, y, z) — the ear gains G1l, G1r and the whole per-ear delays d1l, d1r (0..63 frames) — over `frames`
 * frames, per frame.  With, per ear, G0 the gain in force at that block's first frame (a move in flight: its value there; else the
 * smoother's output), D0 the delay there as an unsigned 32.32 number (at rest d << 32), N = frames, and k the frames of the move
 * rendered so far:
 *   inc = (int64)((d1 << 32) - D0) / (int64)N   (truncated toward zero),   both smoothers are put at rest at the target gains
 *   frame t = k + j < N:  g = clamp(G0 + ((G1 - G0) * ((float)t / (float)N)), min(G0, G1), max(G0, G1)),   D = D0 + t * inc
 *   frame t >= N:         g = G1,   D = d1 << 32 exactly
 *   q = D >> 32,  f = (float)((uint32_t)D >> 8) * 2^-24,  a = m[i - q],  x = f == 0 ? a : a + ((m[i - q - 1] - a) * f),  out = x * g
 * every operation a separately rounded f32 operation, the division IEEE, no FMA; m is the mono row with its 64 frames of history.  D
 * stays between D0 and d1 << 32, so f != 0 implies q <= 62.  Behind a rendered block k += the block's frames; once k >= N the node is
 * at rest at the target, bit for bit a spatialiser set there whose smoothers have settled.  There is no silence shortcut: a move
 * advances in every block.  frames == 0 is a step: it queues the three messages that the last of three param calls for that position queues.  A second move starts from where the first stands;
 * a param 0 / 1 / 2 during a move ends it: the gains glide on from the move's current values on the smoothers, the delays step.
 * Several messages for one block apply in send order.  A voice inside a move is not steady: its calls run the control kernel, and
 * lazy calls resume with the first call behind the move.  The node's position as params 0..2 see it is the move's target from this
 * call on.  FWGPU_ERR_INVALID for a node of another kind, a NaN coordinate, or frames > FWGPU_SPATIAL_MOVE_FRAMES_MAX. */
#define FWGPU_SPATIAL_MOVE_FRAMES_MAX 16777216
int fwgpu_spatial_move(fwgpu_ctx* ctx, int64_t node, float x, float y, float z, uint32_t frames, uint32_t at_block);

/* ---- biquad: a coefficient sweep (a moving cutoff) in one message (SPEC).
 * fwgpu_biquad_sweep: from the first frame of block `at_block` of the next process call, move the node's five coefficients
 * (b0, b1, b2, a1, a2) to the ones params 1 and 2 would set for `cutoff_hz` and `q` — T, computed in f64 with the same clamps and
 * rounded to f32 — over `frames` frames, linearly and per frame.  With A the five values the filter has reached at that block's first
 * frame, d_i = T_i - A_i (one f32 subtraction), N = frames and k the frames of the sweep rendered so far, the frame j frames ahead uses
 *   c_i(j) = k + j >= N ? T_i : clamp(A_i + (d_i * ((float)(k + j) / (float)N)), min(A_i, T_i), max(A_i, T_i))
 * every operation a separately rounded f32 operation, the division IEEE, no FMA; the filter itself is what it is at rest, frame by
 * frame with that frame's values: ff = ((b0*x) + (b1*x1)) + (b2*x2); y = fma(-a1, y1, fma(-a2, y2, ff)).  Behind a rendered block
 * k += the block's frames; once k >= N the node is at rest at T.  The stable (a1, a2) form a convex set, so every frame of a sweep
 * between two stable filters is a stable filter; a long sweep that must follow log-frequency is several segments.
 * frames == 0 is exactly params 1 + 2 (a step).  A second sweep starts from where the first stands; params 1 / 2 during a sweep end it
 * and set the coefficients; several messages for one block apply in send order.  A filter inside a sweep is not steady: its calls run
 * the control kernel, and lazy calls resume with the first call behind the sweep.  The node's cutoff and Q as params 1 / 2 see them are
 * the sweep's targets from this call on.  FWGPU_ERR_INVALID for a node of another kind, a NaN cutoff_hz or q, or frames >
 * FWGPU_BIQUAD_SWEEP_FRAMES_MAX. */
#define FWGPU_BIQUAD_SWEEP_FRAMES_MAX 16777216
int fwgpu_biquad_sweep(fwgpu_ctx* ctx, int64_t node, float cutoff_hz, float q, uint32_t frames, uint32_t at_block);

/* ProcInfo::stream_time_secs / stream_status (core/node.rs:111-132) of the most recent fwgpu_process_interleaved call —
 * what a custom node run through fwgpu_node_process inside that call would be handed — and how often the backend has
 * reported StreamStatus::OUTPUT_UNDERFLOW (bit 1) / INPUT_OVERFLOW (bit 0) so far.  Any pointer may be NULL. */
int fwgpu_proc_info(fwgpu_ctx* ctx, double* stream_time_secs, uint32_t* stream_status, uint64_t* output_underflows,
                    uint64_t* input_overflows);

/* ---- headless stream: the reference's audio-backend callback without a device (firewheel-cpal/src/lib.rs:378-449
 * DataCallback::callback; its non-cpal "dummy backend" is todo!() at lib.rs:150,168,222).  The caller plays the backend:
 * it calls fwgpu_stream_callback once per device period with the instant of that callback on ITS clock (cpal's
 * info.timestamp().callback).  The stream-time and underflow bookkeeping is the reference's, line for line: the first
 * callback's instant is ignored (stream time 0), the second one anchors the clock, and from then on a callback that
 * arrives later than the previous one's stream time + 1.2 periods is an OUTPUT_UNDERFLOW, passed on as stream_status. */
typedef struct fwgpu_stream fwgpu_stream;
fwgpu_stream* fwgpu_stream_open(fwgpu_ctx* ctx, uint32_t num_in_channels, uint32_t num_out_channels);
void fwgpu_stream_close(fwgpu_stream* s);
/* returns the StreamStatus bits handed to process_interleaved (>= 0) or a negative error; `output` is always filled */
int fwgpu_stream_callback(fwgpu_stream* s, float* output, uint64_t frames, double callback_instant_secs);
int fwgpu_stream_stats(fwgpu_stream* s, uint64_t* callbacks, uint64_t* underflows, double* last_stream_time_secs);
/* The backend thread's loop without the device: `n_callbacks` callbacks of `frames` frames back to back, callback i at
 * instant first_instant_secs + i * frames / sample_rate — a stream that never underruns, driven as fast as the engine
 * answers.  `output` (frames x num_out_channels) is overwritten by every callback and holds the last block on return.
 * *elapsed_secs (may be NULL) = wall time of the loop on the monotonic clock: elapsed / n_callbacks is what one callback
 * costs the audio thread, with nothing of the caller's language runtime inside the loop.  Returns 0 or the first error. */
int fwgpu_stream_run(fwgpu_stream* s, float* output, uint64_t frames, uint32_t n_callbacks, double first_instant_secs,
                     double* elapsed_secs);

/* AudioNodeProcessor::process (core/node.rs:37-53) for ONE activated node on caller (host) buffers —
 * the literal per-node drop-in for graph/processor.rs:243.  inputs/outputs: arrays of `frames` floats.
 * out_silence_mask is pre-set by the caller (the reference passes 0). */
int fwgpu_node_process(fwgpu_ctx* ctx, int64_t node, uint64_t frames, const float* const* inputs,
                       uint32_t num_inputs, float* const* outputs, uint32_t num_outputs,
                       uint64_t in_silence_mask, uint64_t* out_silence_mask, double stream_time_secs,
                       uint32_t stream_status);

/* ---- measurement hooks (bench.py): HIP-event timing of the dominant kernel on the ctx stream */
int fwgpu_timing_enable(fwgpu_ctx* ctx, int on);
/* which: 0 = fused leaf kernel (k_leaf_sum / k_chain, dominant), 1 = control kernel, 2 = upper/out kernels,
 * 3 = all kernels of one generic-executor block, 4 = k_fir_gemm alone (FIR banks).
 * Returns accumulated milliseconds and launch count since the last reset. */
int fwgpu_timing_read(fwgpu_ctx* ctx, int which, double* total_ms, uint64_t* launches);
int fwgpu_timing_reset(fwgpu_ctx* ctx);
/* device facts for the bench line */
int fwgpu_device_info(fwgpu_ctx* ctx, char* name, int name_cap, int* compute_units, uint64_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* FWGPU_H */
