// TEST DOUBLE'S COMPANION (tests/test_stream_source.py), header-only access beside the harness library, built on its own with the
// harness's include paths and flags:
//   - the messages a host-only ctx keeps for nodes that no built plan holds yet (early_peek.h), and the bytes of a stream's
//     ring (the fake runtime's device memory is host memory);
//   - the stream's ONE statement (fwgpu_types.h smp_stream_*, the functions the kernels compile) on the host, driven block by block
//     with the looping sampler's playhead move restated here (k_common.hip.h sampler_advance is device code).
#include "early_peek.h"

// the ring of stream `sample`: `n` bytes from byte `off` (0: no such stream, or out of range)
extern "C" int ssp_ring_bytes(const fwgpu_ctx* c, int sample, unsigned long long off, unsigned long long n, unsigned char* out) {
    if (!c || sample < 0 || sample >= (int)c->samples.size() || c->samples[sample].stream < 0 || !c->samples[sample].desc.data) return 0;
    const fwgpu::SampleDesc& d = c->samples[sample].desc;
    const unsigned long long bytes = d.frames * (unsigned long long)d.channels * ((d.format == fwgpu::FMT_I_F32 || d.format == fwgpu::FMT_P_F32) ? 4u : 2u);
    if (off > bytes || n > bytes - off) return 0;
    memcpy(out, (const unsigned char*)d.data + off, n);
    return 1;
}
// what the control side holds for stream `sample`: out = {written, consumed, starved, ended, end_at, finished, detached, pub + 1, ring}
extern "C" int ssp_stream_rec(const fwgpu_ctx* c, int sample, unsigned long long* out) {
    if (!c || sample < 0 || sample >= (int)c->samples.size() || c->samples[sample].stream < 0) return 0;
    const fwgpu::StreamRec& r = c->streams[c->samples[sample].stream];
    out[0] = r.written, out[1] = r.consumed, out[2] = r.starved, out[3] = r.ended, out[4] = r.end_at, out[5] = r.finished, out[6] = r.detached;
    out[7] = (unsigned long long)(r.pub + 1), out[8] = r.ring;
    return 1;
}
extern "C" int ssp_stream_pub_n(const fwgpu_ctx* c) { return c ? c->stream_pub_n : -1; }

// ---- the state machine.  `st`: a whole NodeState (128 bytes) the caller keeps
static_assert(sizeof(fwgpu::NodeState) == 128, "the caller's buffer");
extern "C" void ssp_init(void* st) {
    fwgpu::NodeState s;
    memset(&s, 0, sizeof(s));
    s.sample = -1;
    fwgpu::smp_env_reset(s);
    memcpy(st, &s, sizeof(s));
}
extern "C" void ssp_bind(void* st, int sample, unsigned long long R, unsigned long long W, int stop_playback) {
    fwgpu::NodeState& s = *(fwgpu::NodeState*)st;
    s.sample = sample;
    fwgpu::smp_stream_bind(s, R, W);
    if (stop_playback) {
        s.playhead = s.has_loop ? s.loop_start : 0;
        s.playing = 0;
        fwgpu::smp_env_reset(s);
    }
}
extern "C" void ssp_unbind(void* st, int sample) {
    fwgpu::NodeState& s = *(fwgpu::NodeState*)st;
    s.sample = sample;
    if (fwgpu::smp_stream_on(s)) fwgpu::smp_stream_unbind(s);
}
extern "C" void ssp_msg(void* st, unsigned long long W, int has_end, unsigned long long E) {
    fwgpu::smp_stream_msg(*(fwgpu::NodeState*)st, W, has_end, E);
}
// what = 0 play, 1 pause, 2 stop
extern "C" void ssp_transport(void* st, int what) {
    fwgpu::NodeState& s = *(fwgpu::NodeState*)st;
    if (what == 0) {
        if (!fwgpu::smp_stream_finished(s)) s.playing = 1;
    } else if (what == 1) {
        fwgpu::smp_pause(s);
    } else {
        fwgpu::smp_stop(s);
    }
}
// one block of n frames behind the block's messages; muted: the gain rests below 1e-5 (the playhead holds).  Returns 0: the sampler
// does not play, 1: starved, 2 | data << 8: rendered, `data` frames of it in front of the end
extern "C" unsigned ssp_block(void* st, unsigned n, int muted) {
    fwgpu::NodeState& s = *(fwgpu::NodeState*)st;
    if (s.sample < 0 || !s.playing) return 0u;
    if (fwgpu::smp_stream_starved(s, n)) return 1u;
    const uint64_t ph0 = s.playhead;
    const unsigned data = fwgpu::smp_stream_block_data(s, n);
    if (!muted && s.has_loop && s.loop_start < s.loop_end) {  // the looping sampler's move (sampler.rs:445-484: one wrap per block)
        if (s.playhead >= s.loop_end) s.playhead = s.loop_start;
        const uint64_t left = s.loop_end - s.playhead;
        if (left < (uint64_t)n) s.playhead = s.loop_start + ((uint64_t)n - left);
        else s.playhead += (uint64_t)n;
    }
    fwgpu::smp_env_behind_block(s, n);
    fwgpu::smp_stream_behind_block(s, ph0, n);
    return 2u | (data << 8);
}
// out = {W, C, E, U, flags, playing, playhead, has_loop, loop_start, loop_end}
extern "C" void ssp_get(const void* st, unsigned long long* out) {
    const fwgpu::NodeState& s = *(const fwgpu::NodeState*)st;
    const fwgpu::SmpStream t = fwgpu::smp_stream_of(s);
    out[0] = t.W, out[1] = t.C, out[2] = t.E, out[3] = t.U, out[4] = t.flags, out[5] = (unsigned long long)s.playing, out[6] = s.playhead;
    out[7] = (unsigned long long)s.has_loop, out[8] = s.loop_start, out[9] = s.loop_end;
}
