"""Host-side mirror of the reference interface for the accelerated path, over the C ABI.

Names, argument meaning and error behaviour follow the reference (BillyDM/firewheel @ 2024-10-16):
  * `FirewheelGpuCtx`   ~ FirewheelGraphCtx + FirewheelProcessor (graph/context.rs:29-254, graph/processor.rs:18-248)
  * graph methods       ~ AudioGraph (graph/graph.rs:198-580): add_node, remove_node, connect, disconnect, ...
  * node classes        ~ basic_nodes (nodes/*.rs): constructors take the same arguments; the control-half
                          setters (set_percent_volume, play, ...) become messages with an `at_block` tag.
All arithmetic happens in libfwgpu's HIP kernels; this file only marshals arguments.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import FwgpuError


class SampleFormat:  # core/sample_resource.rs:28-335
    INTERLEAVED_I16, INTERLEAVED_U16, INTERLEAVED_F32, PLANAR_I16, PLANAR_U16, PLANAR_F32 = range(6)
    DTYPE = {0: np.int16, 1: np.uint16, 2: np.float32, 3: np.int16, 4: np.uint16, 5: np.float32}


_ADD_EDGE = {-1: "SrcNodeNotFound", -2: "DstNodeNotFound", -3: "InPortOutOfRange", -4: "OutPortOutOfRange",
             -5: "EdgeAlreadyExists", -6: "InputPortAlreadyConnected", -7: "CycleDetected"}
_COMPILE = {-10: "CycleDetected", -11: "ManyToOneError", -12: "NodeActivationFailed"}


class AddEdgeError(Exception):  # graph/graph/error.rs
    def __init__(self, code):
        super().__init__(_ADD_EDGE.get(code, str(code)))
        self.code = code
        self.name = _ADD_EDGE.get(code, str(code))


class CompileGraphError(Exception):  # graph/graph/error.rs
    def __init__(self, code, msg=""):
        super().__init__("%s: %s" % (_COMPILE.get(code, str(code)), msg))
        self.code = code
        self.name = _COMPILE.get(code, str(code))


class LoopRange:  # nodes/sampler.rs:16-19
    NONE, FULL, RANGE_SECS = 0, 1, 2

    def __init__(self, mode, start=0.0, end=0.0):
        self.mode, self.start, self.end = mode, start, end

    @staticmethod
    def Full():
        return LoopRange(LoopRange.FULL)

    @staticmethod
    def RangeSecs(start, end):
        return LoopRange(LoopRange.RANGE_SECS, start, end)


# ------------------------------------------------------------------------------------------- nodes
class _Node(object):
    KIND = 0
    cx = None
    id = None

    def params(self):
        return []

    def _bind(self, cx, node_id):
        self.cx, self.id = cx, node_id

    def _set(self, param, value, at_block=0):
        self.cx._check(self.cx.L.fwgpu_node_set_param(self.cx.c, self.id, param, value, at_block))


class DummyAudioNode(_Node):  # nodes/dummy.rs
    KIND = 0


class BeepTestNode(_Node):  # nodes/beep_test.rs:14-33
    KIND = 1

    def __init__(self, freq_hz, gain_db, enabled):
        self.freq_hz, self.gain_db, self._enabled = freq_hz, gain_db, enabled

    def params(self):
        return [self.freq_hz, self.gain_db, 1.0 if self._enabled else 0.0]

    def set_enabled(self, enabled, at_block=0):
        self._enabled = enabled
        self._set(0, 1.0 if enabled else 0.0, at_block)


def _gain_ride(node, value, frames, curve, at_block):
    """fwgpu_gain_ride for a VolumeNode / StereoPanNode: `curve` as CrossfadeNode.crossfade_to takes it"""
    shape, (x1, y1, x2, y2) = (0, (0.0, 0.0, 1.0, 1.0)) if curve is None else (1, curve)
    node.cx._check(node.cx.L.fwgpu_gain_ride(node.cx.c, node.id, value, frames, shape, x1, y1, x2, y2, at_block))


class VolumeNode(_Node):  # nodes/volume.rs:14-39
    KIND = 2

    def __init__(self, percent_volume):
        self.percent_volume = max(percent_volume, 0.0)

    def params(self):
        return [self.percent_volume]

    def set_percent_volume(self, percent_volume, at_block=0):
        self.percent_volume = max(percent_volume, 0.0)
        self._set(0, percent_volume, at_block)

    RIDE_FRAMES_MAX = 1 << 24

    def ride_to(self, percent_volume, frames, curve=None, at_block=0):
        """from block `at_block` of the next process call on, ride the gain from where it stands to what `percent_volume` sets, over
        `frames` frames (0: a hard set with no 10 ms glide) along `curve` — None: linear; (x1, y1, x2, y2): the cubic Bezier
        CrossfadeNode.crossfade_to takes.  ONE message instead of a set_percent_volume per block (fwgpu_gain_ride): the music bus down
        to 30 % over two seconds with an ease is `music.ride_to_secs(30.0, 2.0, (0.42, 0.0, 0.58, 1.0))`.  A second ride starts where
        the first stands; set_percent_volume during a ride ends it and glides on from its current value"""
        _gain_ride(self, percent_volume, frames, curve, at_block)
        self.percent_volume = max(percent_volume, 0.0)

    def ride_to_secs(self, percent_volume, secs, curve=None, at_block=0):
        """ride_to with the length in seconds of the context's sample rate"""
        self.ride_to(percent_volume, max(0, int(round(secs * self.cx.sample_rate))), curve, at_block)


class SumNode(_Node):  # nodes/sum.rs
    KIND = 3


class SamplerNode(_Node):  # nodes/sampler.rs:46-182
    KIND = 4

    def __init__(self, percent_volume):
        self.percent_volume = max(percent_volume, 0.0)
        self.playing = False

    def params(self):
        return [self.percent_volume]

    def set_percent_volume(self, percent_volume, at_block=0):
        self.percent_volume = max(percent_volume, 0.0)
        self._set(0, percent_volume, at_block)

    def set_sample(self, sample, stop_playback, at_block=0):
        """`sample`: a sample id, or a StreamSource (FirewheelGpuCtx.new_stream) — that binds the stream to this sampler, once"""
        sid = sample.id if isinstance(sample, StreamSource) else sample
        self.cx._check(self.cx.L.fwgpu_sampler_set_sample(self.cx.c, self.id, sid, int(stop_playback), at_block))

    def play(self, at_block=0):  # sampler.rs:82-97: only sends when not already playing
        if not self.playing:
            self.cx._check(self.cx.L.fwgpu_sampler_play(self.cx.c, self.id, at_block))
            self.playing = True

    def pause(self, at_block=0):
        if self.playing:
            self.cx._check(self.cx.L.fwgpu_sampler_pause(self.cx.c, self.id, at_block))
            self.playing = False

    def stop(self, at_block=0):
        if self.playing:
            self.cx._check(self.cx.L.fwgpu_sampler_stop(self.cx.c, self.id, at_block))
            self.playing = False

    def is_playing(self):  # sampler.rs:162-164: the control half's own flag, not the processor's
        return self.playing

    def set_playhead(self, playhead_secs, at_block=0):
        self.cx._check(self.cx.L.fwgpu_sampler_set_playhead_secs(self.cx.c, self.id, playhead_secs, at_block))

    def set_loop_range(self, loop_range, at_block=0):
        lr = loop_range or LoopRange(LoopRange.NONE)
        self.cx._check(self.cx.L.fwgpu_sampler_set_loop_range(self.cx.c, self.id, lr.mode, lr.start, lr.end, at_block))

    # ---- SPEC gain envelope: declicked pause, stop and start in one message each
    FADE_FRAMES_MAX = 1 << 24
    FADE_THEN = {None: 0, "none": 0, "pause": 1, "stop": 2}

    def fade_to(self, gain, frames, then=None, at_block=0):
        """from block `at_block` of the next process call on, move the voice's gain envelope to `gain` (0..1) over `frames` frames,
        linearly (0: a step); `then` = None, "pause" or "stop": what the sampler does at the fade's end (fwgpu_sampler_fade).  The
        envelope is a transient — every pause and stop puts it back to 1.0 — so a level that should last belongs in percent_volume.
        With a `then`, is_playing() is False from this call on, as after pause() / stop(): the voice is on its way out."""
        if then not in self.FADE_THEN:
            raise ValueError("fade_to: then must be None, 'pause' or 'stop'")
        self.cx._check(self.cx.L.fwgpu_sampler_fade(self.cx.c, self.id, gain, frames, self.FADE_THEN[then], at_block))
        if self.FADE_THEN[then]:
            self.playing = False

    def fade_to_secs(self, gain, secs, then=None, at_block=0):
        """... over `secs` seconds, rounded to whole frames of the context's sample rate"""
        self.fade_to(gain, max(0, int(round(secs * self.cx.sample_rate))), then, at_block)

    def fade_out(self, frames, then="stop", at_block=0):
        """a declicked stop (or pause): down to 0 over `frames` frames, then `then`"""
        self.fade_to(0.0, frames, then, at_block)

    def fade_in(self, frames, at_block=0):
        """a declicked start of a voice that is not playing — three messages for one block: the envelope steps to 0, the voice
        plays, the envelope rises to 1 over `frames` frames"""
        self.fade_to(0.0, 0, None, at_block)
        self.cx._check(self.cx.L.fwgpu_sampler_play(self.cx.c, self.id, at_block))
        self.playing = True
        self.fade_to(1.0, frames, None, at_block)


class StreamSource(object):
    """A sample whose storage is a ring fed while one sampler plays it (SPEC streaming source; include/fwgpu.h
    fwgpu_sample_create_stream).  `id` is its sample id: destroy_sample / sample_retired take it like any other."""

    def __init__(self, cx, fmt, channels, ring_frames):
        self.cx, self.fmt, self.channels, self.ring_frames = cx, fmt, channels, int(ring_frames)
        self.id = cx._check(cx.L.fwgpu_sample_create_stream(cx.c, fmt, channels, self.ring_frames))
        self.ended = False

    def write(self, data):
        """append frames: a numpy array (or anything numpy converts) laid out as new_sample's data, or a torch tensor on this device
        (no copy through the host).  Returns the frames accepted, 0..frames: the ring's free space as of the last process call known to
        be complete.  A full message ring raises FwgpuError(FWGPU_ERR_QUEUE_FULL); the same call can then be repeated."""
        if hasattr(data, "data_ptr") and getattr(data, "is_cuda", False):
            t = data.contiguous()
            if t.element_size() != np.dtype(SampleFormat.DTYPE[self.fmt]).itemsize:
                raise ValueError("StreamSource.write: the tensor's element size does not fit the stream's format")
            frames = t.numel() // self.channels
            import torch

            torch.cuda.current_stream(t.device).synchronize()  # (the copy runs on the library's own stream)
            return self.cx._check(self.cx.L.fwgpu_sample_stream_write_device(self.cx.c, self.id, C.c_void_p(t.data_ptr()), frames))
        a = np.ascontiguousarray(np.asarray(data, dtype=SampleFormat.DTYPE[self.fmt]))
        frames = a.size // self.channels
        return self.cx._check(self.cx.L.fwgpu_sample_stream_write(self.cx.c, self.id, a.ctypes.data_as(C.c_void_p), frames))

    def end(self):
        """no more data: the sampler stops behind the last frame written.  FwgpuError(FWGPU_ERR_QUEUE_FULL) while the ring has no room
        for the max_block_frames of padding yet"""
        self.cx._check(self.cx.L.fwgpu_sample_stream_end(self.cx.c, self.id))
        self.ended = True

    def status(self):
        """(written, consumed, starved_blocks, finished) as of the last completed process call; never blocks"""
        w, c, u, f = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        self.cx._check(self.cx.L.fwgpu_sample_stream_status(self.cx.c, self.id, C.byref(w), C.byref(c), C.byref(u), C.byref(f)))
        return w.value, c.value, u.value, bool(f.value)

    def free_frames(self):
        """how many frames write() would accept now (an underestimate, never an overestimate; 0 behind end())"""
        w, c, _, fin = self.status()
        return 0 if fin or self.ended else self.ring_frames - (w - c)


class HardClipNode(_Node):  # nodes/hard_clip.rs:7-13
    KIND = 5

    def __init__(self, threshold_db):
        self.threshold_db = threshold_db

    def params(self):
        return [self.threshold_db]


class MonoToStereoNode(_Node):  # nodes/mono_to_stereo.rs
    KIND = 6


class StereoToMonoNode(_Node):  # nodes/stereo_to_mono.rs
    KIND = 7


class StereoPanNode(_Node):  # SPEC node: constant-power pan, pan in [-1, 1]
    KIND = 8

    def __init__(self, pan):
        self.pan = pan

    def params(self):
        return [self.pan]

    def set_pan(self, pan, at_block=0):
        self.pan = pan
        self._set(0, pan, at_block)

    RIDE_FRAMES_MAX = 1 << 24

    def ride_to(self, pan, frames, curve=None, at_block=0):
        """from block `at_block` of the next process call on, ride both ear gains from where they stand to what `pan` sets, over
        `frames` frames (0: a hard set) along `curve` (as VolumeNode.ride_to).  The ride travels in the gains, each ear on its own: a
        ride from hard left to hard right dips in power at the middle — one that must hold power is two rides through the centre"""
        _gain_ride(self, pan, frames, curve, at_block)
        self.pan = pan

    def ride_to_secs(self, pan, secs, curve=None, at_block=0):
        """ride_to with the length in seconds of the context's sample rate"""
        self.ride_to(pan, max(0, int(round(secs * self.cx.sample_rate))), curve, at_block)


class StereoWidthNode(_Node):  # SPEC node: mid/side width, w >= 0 (1 = unchanged, 0 = mono), smoothed
    KIND = 9

    def __init__(self, width):
        self.width = width

    def params(self):
        return [self.width]

    def set_width(self, width, at_block=0):
        self.width = width
        self._set(0, width, at_block)


class BiquadNode(_Node):  # SPEC node: RBJ biquad, Direct Form I in f32; coefficients computed on the control side (f64)
    KIND = 10
    LOWPASS, HIGHPASS, BANDPASS = 0, 1, 2

    def __init__(self, filter_type, cutoff_hz, q=0.70710678):
        self.filter_type, self.cutoff_hz, self.q = filter_type, cutoff_hz, q

    def params(self):
        return [float(self.filter_type), self.cutoff_hz, self.q]

    def set_cutoff_hz(self, cutoff_hz, at_block=0):
        self.cutoff_hz = cutoff_hz
        self._set(1, cutoff_hz, at_block)

    def set_q(self, q, at_block=0):
        self.q = q
        self._set(2, q, at_block)

    SWEEP_FRAMES_MAX = 1 << 24

    def sweep_to(self, cutoff_hz, frames, q=None, at_block=0):
        """from block `at_block` of the next process call on, move the filter to (`cutoff_hz`, `q`; q None: the Q it has) over
        `frames` frames — the five coefficients travel linearly and per frame (0: a step, as set_cutoff_hz) — ONE message for an
        occlusion or under-water muffle instead of a set_cutoff_hz per block (fwgpu_biquad_sweep).  A second sweep starts from where
        the first stands.  `self.cutoff_hz` and `self.q` hold the TARGET from this call on."""
        q = self.q if q is None else q
        self.cx._check(self.cx.L.fwgpu_biquad_sweep(self.cx.c, self.id, cutoff_hz, q, frames, at_block))
        self.cutoff_hz, self.q = cutoff_hz, q

    def sweep_to_secs(self, cutoff_hz, secs, q=None, at_block=0):
        """sweep_to with the length in seconds of the context's sample rate"""
        self.sweep_to(cutoff_hz, max(0, int(round(secs * self.cx.sample_rate))), q, at_block)


class DelayNode(_Node):  # SPEC node: integer-sample delay line (fixed length) with feedback and dry/wet mix
    KIND = 11

    def __init__(self, delay_secs, feedback=0.0, mix=0.5):
        self.delay_secs, self.feedback, self.mix = delay_secs, feedback, mix

    def params(self):
        return [self.delay_secs, self.feedback, self.mix]

    def set_feedback(self, feedback, at_block=0):
        self.feedback = feedback
        self._set(1, feedback, at_block)

    def set_mix(self, mix, at_block=0):
        self.mix = mix
        self._set(2, mix, at_block)


class FirReverbNode(_Node):  # SPEC node: convolution with an impulse-response sample (f32 MFMA Toeplitz GEMM)
    KIND = 12

    def __init__(self, ir, ir_b=None, max_taps=0, position=0.0, law=1, morph=None):
        """ir alone: the plain node.  Anything else given: a morph-capable node (SPEC FIR morph, include/fwgpu.h) — slot A = ir, slot
        B = ir_b (None: empty), both zero-padded to max_taps (0: the longer of the two), blended at `position` (0 = A, 1 = B) under
        `law` (0 linear, 1 equal power).  morph=True asks for a morph-capable node whatever the other arguments are — with ir_b=None
        and the defaults that is the wet fader, a node with an empty slot B; morph=None (default) decides as above"""
        self.ir, self.ir_b, self.max_taps, self.position, self.law = ir, ir_b, max_taps, position, law
        self.morph = bool(morph) if morph is not None else not (ir_b is None and max_taps == 0 and position == 0.0 and law == 1)
        if not self.morph and not (ir_b is None and max_taps == 0 and position == 0.0 and law == 1):
            raise ValueError("FirReverbNode: morph=False with ir_b, max_taps, position or law given")

    def params(self):
        if not self.morph:
            return [float(self.ir)]
        return [float(self.ir), float(-1 if self.ir_b is None else self.ir_b), float(self.max_taps), float(self.position), float(self.law)]

    def morph_to(self, position, frames, curve=None, at_block=0):
        """from block `at_block` of the next process call on, move to `position` over `frames` frames (0: a jump) along `curve`
        (None: linear; else the Bezier's (x1, y1, x2, y2)) — fwgpu_fir_morph"""
        shape, (x1, y1, x2, y2) = (0, (0.0, 0.0, 1.0, 1.0)) if curve is None else (1, curve)
        self.cx._check(self.cx.L.fwgpu_fir_morph(self.cx.c, self.id, position, frames, shape, x1, y1, x2, y2, at_block))
        self.position = position

    def morph_to_secs(self, position, secs, curve=None, at_block=0):
        """... over `secs` seconds, rounded to whole frames of the context's sample rate"""
        self.morph_to(position, max(0, int(round(secs * self.cx.sample_rate))), curve, at_block)

    def set_ir(self, slot, sample):
        """exchange the impulse response of a slot nobody hears (0 = A, 1 = B; sample None: empty slot B); takes effect with the next
        update — fwgpu_fir_set_ir"""
        self.cx._check(self.cx.L.fwgpu_fir_set_ir(self.cx.c, self.id, slot, -1 if sample is None else sample))
        if slot == 0:
            self.ir = sample
        else:
            self.ir_b = sample


class ResamplerNode(_Node):  # SPEC node: resampling source — polyphase windowed sinc, 32.32 fixed-point position
    KIND = 13

    def __init__(self, sample, ratio=1.0, loop=False, playing=True):
        self.sample, self.ratio, self.loop, self.playing = sample, ratio, loop, playing

    def params(self):
        return [float(self.sample), self.ratio, 1.0 if self.loop else 0.0, 1.0 if self.playing else 0.0]

    def set_ratio(self, ratio, at_block=0):
        """source frames consumed per output frame (= source rate / stream rate x playback speed)"""
        self.ratio = ratio
        self._set(1, ratio, at_block)

    def set_playing(self, playing, at_block=0):
        self.playing = playing
        self._set(3, 1.0 if playing else 0.0, at_block)

    def seek_frames(self, frame, at_block=0):
        self._set(4, float(frame), at_block)

    GLIDE_FRAMES_MAX = 1 << 24

    def glide_to(self, ratio, frames, at_block=0):
        """from block `at_block` of the next process call on, move the ratio to `ratio` over `frames` output frames, linearly in the
        32.32 step (0: a step, as set_ratio) — ONE message for a pitch that moves every frame (Doppler: see doppler_ratio).
        `self.ratio` holds the TARGET from this call on, also while the node is still on its way there."""
        self.cx._check(self.cx.L.fwgpu_resampler_glide(self.cx.c, self.id, ratio, frames, at_block))
        self.ratio = ratio


def doppler_ratio(base_ratio, radial_speed, speed_of_sound=343.0):
    """the ratio of a source that moves at `radial_speed` along the line to the listener (same unit as `speed_of_sound`, > 0:
    receding, the pitch drops): base_ratio * c / (c + v).  A source closing at the speed of sound or faster has no ratio."""
    c, v = float(speed_of_sound), float(radial_speed)
    if not c > 0.0 or not v > -c:
        raise ValueError("doppler_ratio: radial_speed must be greater than -speed_of_sound (and speed_of_sound positive)")
    return base_ratio * c / (c + v)


class SpatialNode(_Node):  # SPEC node: 3D spatialiser — distance gain, equal-power pan, per-ear delay
    KIND = 14

    def __init__(self, x, y, z):
        self.pos = [x, y, z]

    def params(self):
        return list(self.pos)

    def set_position(self, x, y, z, at_block=0):
        """source position relative to the listener: +x right, +y up, -z forward"""
        self.pos = [x, y, z]
        for i, v in enumerate(self.pos):
            self._set(i, v, at_block)

    MOVE_FRAMES_MAX = 1 << 24

    def move_to(self, x, y, z, frames, at_block=0):
        """from block `at_block` of the next process call on, move the source to (x, y, z) over `frames` frames (0: a step, as
        set_position): the ear gains travel linearly and per frame and the per-ear delays glide as 32.32 fractions of a frame, read
        with a two-tap blend — ONE message for a source that crosses the stereo image without a click, instead of a set_position
        per block, whose whole-frame delays step (fwgpu_spatial_move).  A second move starts from where the first stands; a
        set_position during a move ends it.  `self.pos` holds the TARGET from this call on.  A fly-by moves place and pitch in the
        same tick, the spatialiser and the resampling source in front of it:

            spat.move_to(+8.0, 0.0, -2.0, frames)                                  # from the left of the listener to the right
            src.glide_to(doppler_ratio(1.0, radial_speed_at_the_end), frames)      # ... while the pitch drops
        """
        self.cx._check(self.cx.L.fwgpu_spatial_move(self.cx.c, self.id, x, y, z, frames, at_block))
        self.pos = [x, y, z]

    def move_to_secs(self, x, y, z, secs, at_block=0):
        """move_to with the length in seconds of the context's sample rate"""
        self.move_to(x, y, z, max(0, int(round(secs * self.cx.sample_rate))), at_block)


class HostNode(_Node):
    """any other `dyn AudioNodeProcessor` (graph/processor.rs:243) inside a device-resident graph: `process` runs on the host,
    on the audio thread, once per block — process(frames, inputs, outputs, in_silence_mask, stream_time_secs, stream_status)
    -> out_silence_mask, inputs / outputs being float32 numpy views (FWGPU_HOST_NODE, include/fwgpu.h)"""
    KIND = 15

    def __init__(self, process):
        self.process = process
        self._cb = _lib.host_process_adapter(process)

    def _bind(self, cx, node_id):
        super()._bind(cx, node_id)
        cx._check(cx.L.fwgpu_host_node_set_process(cx.c, node_id, self._cb, None))


METER_DTYPE = np.dtype([("peak", np.float32), ("sum_squares", np.float32), ("over", np.uint32), ("frames", np.uint32)])  # fwgpu_meter_reading


class MeterNode(_Node):
    """SPEC node: level meter — per block and input channel the peak, the sum of squares and the number of
    samples over 1.0, measured on the device.  add_node(n, n, MeterNode()) passes the audio through, add_node(n, 0, ...) is a tap.
    `ring_blocks` (1..65536) = how many blocks of readings the node retains for `read` / FirewheelGpuCtx.meter_read.
    With `fft_size` (256, 512, 1024, 2048 or 4096; at most 8 channels) the node is a spectrum meter as well: per block and input channel
    the band powers of a Hann-windowed FFT over the channel's last fft_size frames, `bands` log-spaced bands over bins 1..fft_size/2
    (0: every bin, DC included), read by `spectrum` / FirewheelGpuCtx.spectrum_read"""
    KIND = 16

    def __init__(self, ring_blocks=1024, fft_size=None, bands=32):
        self.ring_blocks = ring_blocks
        self.fft_size = fft_size
        self.bands = bands

    def params(self):
        if self.fft_size is None:
            return [float(self.ring_blocks)]
        return [float(self.ring_blocks), float(self.fft_size), float(self.bands)]

    def read(self, first_block, num_blocks):
        return self.cx.meter_read(self.id, first_block, num_blocks)

    def spectrum(self, first_block, num_blocks):
        return self.cx.spectrum_read(self.id, first_block, num_blocks)

    @staticmethod
    def band_edges(fft_size, bands):
        """the SPEC's edges e[0..B]: band b covers bins e[b] .. e[b+1] - 1 (bands == 0: B = fft_size/2 + 1, e[b] = b)"""
        M = fft_size // 2
        if bands == 0:
            return np.arange(M + 2, dtype=np.uint32)
        e = [1]
        for b in range(1, bands):
            e.append(max(e[-1] + 1, min(M + 1 - (bands - b), int(math.floor(math.pow(float(M), float(b) / bands) + 0.5)))))
        return np.array(e + [M + 1], dtype=np.uint32)

    @staticmethod
    def band_hz(fft_size, bands, sample_rate):
        """[B][2]: the centre frequencies of each band's first and last bin"""
        e = MeterNode.band_edges(fft_size, bands).astype(np.float64)
        return np.stack([e[:-1], e[1:] - 1.0], axis=1) * (float(sample_rate) / fft_size)

    @staticmethod
    def power_db(power):
        """10 * log10(power), in f32 (0 -> -inf): 0 dB is a full-scale sine on a bin centre"""
        with np.errstate(divide="ignore", invalid="ignore"):
            return (np.float32(10.0) * np.log10(np.asarray(power, dtype=np.float32))).astype(np.float32)

    @staticmethod
    def gain_to_db(amp):
        """core/util.rs gain_to_db: 20 * log10(amp), in f32 (0 -> -inf)"""
        with np.errstate(divide="ignore", invalid="ignore"):
            return (np.float32(20.0) * np.log10(np.asarray(amp, dtype=np.float32))).astype(np.float32)

    @staticmethod
    def db_to_gain(db):
        """core/util.rs db_to_gain: 10 ** (0.05 * db), in f32 — what gain_to_db inverts"""
        return np.power(np.float32(10.0), np.float32(0.05) * np.asarray(db, dtype=np.float32)).astype(np.float32)

    @staticmethod
    def peak_db(readings):
        return MeterNode.gain_to_db(np.asarray(readings)["peak"])

    @staticmethod
    def rms_db(readings):
        """rms = sqrt(sum_squares / frames) through gain_to_db"""
        r = np.asarray(readings)
        with np.errstate(divide="ignore", invalid="ignore"):
            rms = np.sqrt(r["sum_squares"] / r["frames"].astype(np.float32), dtype=np.float32)
        return MeterNode.gain_to_db(rms)


class LimiterNode(_Node):
    """SPEC node: look-ahead limiter — linked channels, brickwall at `ceiling` (linear, 0.001..1000) with a hold of
    `hold_frames` (0..1920), `latency_frames` = 63 frames late.  A sliding minimum of the target gain and a 64-term moving average, no
    recurrence in time: the blocks of a batch render in parallel, bit-exact against the numpy model of tests/test_limiter.py.
    add_node(channels, channels, LimiterNode(...)), channels in 1..8.  `ceiling_db=` gives the ceiling in decibels instead, converted by
    the function MeterNode.peak_db inverts.  No parameters after creation."""
    KIND = 17
    latency_frames = 63

    def __init__(self, ceiling=1.0, hold_frames=128, channels=2, ceiling_db=None):
        self.ceiling = float(MeterNode.db_to_gain(ceiling_db)) if ceiling_db is not None else ceiling
        self.hold_frames = hold_frames
        self.channels = channels

    @property
    def ceiling_db(self):
        return float(MeterNode.gain_to_db(self.ceiling))

    def params(self):
        return [float(self.ceiling), float(self.hold_frames)]


class DuckerNode(_Node):
    """SPEC node: sidechain ducker — while the key bus is above `threshold` (linear, 1e-6..1000) the main bus is
    turned down to `depth` (linear gain while ducked, 0..1): down over `attack_frames`, held for `hold_frames` after the key has gone
    quiet, back up over `release_frames` (1..32768, 1..32768, 0..32768).  The gain is a function of integer counts over windows of the
    key's gate bits, no recurrence in time: the blocks of a batch render in parallel, bit-exact against the numpy model of
    tests/test_ducker.py; no latency.  add_node(channels + key_channels, channels, DuckerNode(...)): inputs 0..channels-1 are the main
    bus, the rest the key, which is never heard; channels and key_channels in 1..8.  `threshold_db=` / `depth_db=` give the two in
    decibels instead, converted by MeterNode.db_to_gain.  No parameters after creation."""
    KIND = 18

    def __init__(self, threshold=0.05, depth=0.25, attack_frames=480, release_frames=12000, hold_frames=4800, channels=2, key_channels=2,
                 threshold_db=None, depth_db=None):
        self.threshold = float(MeterNode.db_to_gain(threshold_db)) if threshold_db is not None else threshold
        self.depth = float(MeterNode.db_to_gain(depth_db)) if depth_db is not None else depth
        self.attack_frames = attack_frames
        self.release_frames = release_frames
        self.hold_frames = hold_frames
        self.channels = channels
        self.key_channels = key_channels

    @property
    def num_inputs(self):
        return self.channels + self.key_channels

    def attack_secs(self, sample_rate):
        return self.attack_frames / float(sample_rate)

    def release_secs(self, sample_rate):
        return self.release_frames / float(sample_rate)

    def hold_secs(self, sample_rate):
        return self.hold_frames / float(sample_rate)

    @classmethod
    def from_secs(cls, sample_rate, attack_secs=0.01, release_secs=0.25, hold_secs=0.1, **kw):
        """the three times in seconds, rounded to whole frames of `sample_rate`"""
        return cls(attack_frames=max(1, int(round(attack_secs * sample_rate))), release_frames=max(1, int(round(release_secs * sample_rate))),
                   hold_frames=max(0, int(round(hold_secs * sample_rate))), **kw)

    def params(self):
        return [float(self.threshold), float(self.depth), float(self.attack_frames), float(self.release_frames), float(self.hold_frames)]


class CompressorNode(_Node):
    """SPEC node: bus compressor — self-keyed, linked channels.  Above `threshold` (linear, 1e-6..1000) the level
    rises `ratio` (1..1000) times slower, through a soft knee `knee_db` wide (0..24); the gain comes down over `attack_frames`, stays for
    `hold_frames` after the level has fallen and comes back over `release_frames` (1..32768, 0..2048, 1..32768); `makeup` (linear,
    0.001..1000) scales the result.  The curve is a table of 16 knots per octave built on the host, the gain a function of integer sums
    over windows of the quantised target, no recurrence in time: the blocks of a batch render in parallel, bit-exact against the numpy
    model of tests/compressor_model.py; no latency.  add_node(channels, channels, CompressorNode(...)), channels in 1..8.
    `threshold_db=` / `makeup_db=` give the two in decibels instead, converted by MeterNode.db_to_gain.  No parameters after creation."""
    KIND = 21
    WIN_MAX, HOLD_MAX, CH_MAX = 32768, 2048, 8
    KNOTS_PER_OCTAVE, OCTAVES = 16, 20

    def __init__(self, threshold=0.25, ratio=4.0, knee_db=6.0, attack_frames=240, release_frames=12000, hold_frames=0, makeup=1.0, channels=2,
                 threshold_db=None, makeup_db=None):
        self.threshold = float(MeterNode.db_to_gain(threshold_db)) if threshold_db is not None else threshold
        self.ratio = ratio
        self.knee_db = knee_db
        self.attack_frames = attack_frames
        self.release_frames = release_frames
        self.hold_frames = hold_frames
        self.makeup = float(MeterNode.db_to_gain(makeup_db)) if makeup_db is not None else makeup
        self.channels = channels

    def attack_secs(self, sample_rate):
        return self.attack_frames / float(sample_rate)

    def release_secs(self, sample_rate):
        return self.release_frames / float(sample_rate)

    def hold_secs(self, sample_rate):
        return self.hold_frames / float(sample_rate)

    @classmethod
    def from_secs(cls, sample_rate, attack_secs=0.005, release_secs=0.25, hold_secs=0.0, **kw):
        """the three times in seconds, rounded to whole frames of `sample_rate`"""
        return cls(attack_frames=max(1, int(round(attack_secs * sample_rate))), release_frames=max(1, int(round(release_secs * sample_rate))),
                   hold_frames=max(0, int(round(hold_secs * sample_rate))), **kw)

    def params(self):
        return [float(self.threshold), float(self.ratio), float(self.knee_db), float(self.attack_frames), float(self.release_frames),
                float(self.hold_frames), float(self.makeup)]

    def knee_start(self):
        """T0: the level at which the knee begins, as the node computes it (f64, rounded to f32)"""
        t, knee = float(np.float32(self.threshold)), float(np.float32(self.knee_db))
        return np.float32(t * math.pow(10.0, -knee / 40.0))

    def table(self):
        """G[0..320]: the gain at the knots u_i = 2^(i // 16) * (1 + (i % 16) / 16) times T0, as the node computes it"""
        knee, slope = float(np.float32(self.knee_db)), 1.0 / float(np.float32(self.ratio)) - 1.0
        G = np.empty(self.KNOTS_PER_OCTAVE * self.OCTAVES + 1, dtype=np.float32)
        for i in range(G.size):
            u = math.ldexp(1.0 + (i % 16) / 16.0, i // 16)
            over = 20.0 * math.log10(u) - knee / 2.0
            gr = 0.0
            if knee > 0.0 and 2.0 * abs(over) <= knee:
                t = over + knee / 2.0
                gr = slope * (t * t) / (2.0 * knee)
            elif over > 0.0:
                gr = slope * over
            G[i] = np.float32(math.pow(10.0, gr / 20.0))
        return G

    def static_gain(self, level):
        """the gain (makeup not included) a steady input of linear `level` settles at, before its quantisation to 16 bits: the table
        curve on the host, for a UI's transfer plot.  level: a number or an array, NaN-free"""
        G, f32 = self.table(), np.float32
        key = np.abs(np.asarray(level, dtype=f32))
        with np.errstate(over="ignore"):
            u = (key / self.knee_start()).astype(f32)
        over = u > f32(1)
        d = np.where(over, u.view(np.uint32).astype(np.int64) - 0x3F800000, 0)
        i = d >> 19
        fr = (d & 0x7FFFF).astype(f32) * f32(2.0 ** -19)
        sat = i >= G.size - 1
        i = np.minimum(i, G.size - 2)
        t = (G[i] + ((G[i + 1] - G[i]).astype(f32) * fr).astype(f32)).astype(f32)
        return np.where(over, np.where(sat, G[-1], t), f32(1)).astype(f32)


class DelayCompNode(_Node):
    """SPEC node: latency compensation — a pure delay of `frames` whole frames (0..8192), a copy with no
    arithmetic: what a bus needs that is summed with a bus a LimiterNode has made 63 frames late.  add_node(channels, channels,
    DelayCompNode(frames)), channels in 1..8.  An output block is flagged silent exactly when the `frames` frames in front of it and the
    block itself were; every block of a batch renders in parallel.  `latency_frames` = frames.  No parameters after creation.
    FirewheelGpuCtx.latency_report says where one is needed, compensate_latency puts them there."""
    KIND = 19
    MAX_FRAMES = 8192

    def __init__(self, frames=63, channels=2):
        self.frames = frames
        self.channels = channels

    @property
    def latency_frames(self):
        return self.frames

    def params(self):
        return [float(self.frames)]


class CrossfadeNode(_Node):
    """SPEC node: crossfader — two buses blended along an automated curve.  add_node(node.num_inputs, channels,
    CrossfadeNode(...)): inputs 0..channels-1 are bus A, inputs channels..2*channels-1 bus B, `channels` outputs, channels in 1..8.
    `position` 0 is all A, 1 all B; `law` LAW_LINEAR (a = 1 - p, b = p) or EQUAL_POWER (a = sqrt(1 - p), b = sqrt(p)).  With bus B left
    unconnected the node is a fader of bus A: crossfade_to(1.0, ...) is a fade-out, crossfade_to(0.0, ...) a fade-in.  The position is
    a pure function of the node's frame count, so a fade in flight renders block-parallel and bit-exact against the numpy model of
    tests/test_crossfade.py; at rest at 0 or 1 the output is a copy of one bus, bit for bit.  No latency."""
    KIND = 20
    LAW_LINEAR, EQUAL_POWER = 0, 1
    SHAPE_LINEAR, SHAPE_BEZIER = 0, 1
    FRAMES_MAX = 1 << 24
    # curves: None / LINEAR, or the two inner control points (x1, y1, x2, y2) of a cubic Bezier easing from (0, 0) to (1, 1)
    LINEAR = None
    EASE_IN = (0.42, 0.0, 1.0, 1.0)
    EASE_OUT = (0.0, 0.0, 0.58, 1.0)
    EASE_IN_OUT = (0.42, 0.0, 0.58, 1.0)

    def __init__(self, position=0.0, law=EQUAL_POWER, channels=2):
        self.position = position
        self.law = law
        self.channels = channels

    @property
    def num_inputs(self):
        return 2 * self.channels

    def params(self):
        return [float(self.position), float(self.law)]

    def crossfade_to(self, position, frames, curve=None, at_block=0):
        """from block `at_block` of the next process call on, move to `position` over `frames` frames (0: a jump) along `curve`"""
        shape, (x1, y1, x2, y2) = (self.SHAPE_LINEAR, (0.0, 0.0, 1.0, 1.0)) if curve is None else (self.SHAPE_BEZIER, curve)
        self.cx._check(self.cx.L.fwgpu_crossfade_to(self.cx.c, self.id, position, frames, shape, x1, y1, x2, y2, at_block))
        self.position = position

    def crossfade_to_secs(self, position, secs, curve=None, at_block=0):
        """... over `secs` seconds, rounded to whole frames of the context's sample rate"""
        self.crossfade_to(position, max(0, int(round(secs * self.cx.sample_rate))), curve, at_block)

    def set_position(self, position, at_block=0):
        """a jump (fwgpu_node_set_param 0)"""
        self._set(0, position, at_block)
        self.position = position


class _RawNode(_Node):
    def __init__(self, kind, params):
        self.KIND = kind
        self._p = list(params)

    def params(self):
        return self._p


# ------------------------------------------------------------------------------------------- context
def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class FirewheelGpuCtx(object):
    """Device-resident graph context.  `stream` is an optional hipStream_t (int) to run on."""

    def __init__(self, sample_rate=48000, max_block_frames=256, num_graph_inputs=0, num_graph_outputs=2, device=0,
                 stream=None):
        self.L = _lib.load_library()
        self.sample_rate = sample_rate
        self.max_block_frames = max_block_frames
        self.c = self.L.fwgpu_ctx_create(device, sample_rate, max_block_frames, num_graph_inputs, num_graph_outputs,
                                         C.c_void_p(stream) if stream else None)
        if not self.c:
            raise FwgpuError(-30, self.L.fwgpu_create_error().decode())
        self._nodes = {}
        self._edges = {}  # (dst node, dst port) -> (src node, src port, edge id): what compensate_latency rewires
        self._limbo = []  # removed HostNodes (their ctypes thunks) until a plan without them is the active one
        self._keep = []

    def close(self):
        if getattr(self, "c", None):
            self.L.fwgpu_ctx_destroy(self.c)
            self.c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise FwgpuError(rc, self.L.fwgpu_last_error(self.c).decode())
        return rc

    # ---- AudioGraph (graph/graph.rs)
    @property
    def graph(self):
        return self

    graph_mut = graph

    def graph_in_node(self):
        return self.L.fwgpu_graph_in_node(self.c)

    def graph_out_node(self):
        return self.L.fwgpu_graph_out_node(self.c)

    def add_node(self, num_inputs, num_outputs, node):
        p = np.asarray(node.params(), dtype=np.float32)
        nid = self.L.fwgpu_add_node(self.c, node.KIND, num_inputs, num_outputs, _fptr(p), len(p))
        self._check(nid)
        node._bind(self, nid)
        node._n_in = num_inputs
        self._nodes[nid] = node
        return nid

    def node(self, node_id):
        return self._nodes.get(node_id)

    node_mut = node

    def remove_node(self, node_id):
        self._check(self.L.fwgpu_remove_node(self.c, node_id))
        self._edges = {k: v for k, v in self._edges.items() if k[0] != node_id and v[0] != node_id}
        n = self._nodes.pop(node_id, None)
        if isinstance(n, HostNode):
            # the running plan (and a pending one) still call the node's ctypes thunk until a plan WITHOUT it is the active one
            # (fwgpu_abi.cpp: "the running plan may hold it until the next plan is adopted"): a thunk freed here is a segfault in
            # the next process call.  It waits in limbo for an update that has been adopted (_reap_limbo).
            self._limbo.append([n, False])

    def _reap_limbo(self, updated=False):
        """drop removed host nodes once a plan built AFTER their removal is the active one: an update has returned since
        (entry[1]) and none is waiting for adoption (fwgpu_plan_pending)"""
        if updated:
            for ent in self._limbo:
                ent[1] = True
        if self._limbo and not self.L.fwgpu_plan_pending(self.c):
            self._limbo = [ent for ent in self._limbo if not ent[1]]

    def connect(self, src_node, src_port, dst_node, dst_port, check_for_cycles=False):
        r = self.L.fwgpu_connect(self.c, src_node, src_port, dst_node, dst_port, 1 if check_for_cycles else 0)
        if r < 0:
            raise AddEdgeError(r)
        self._edges[(dst_node, dst_port)] = (src_node, src_port, r)
        return r

    def disconnect(self, src_node, src_port, dst_node, dst_port):
        done = bool(self.L.fwgpu_disconnect(self.c, src_node, src_port, dst_node, dst_port))
        if done:
            self._edges.pop((dst_node, dst_port), None)
        return done

    def disconnect_by_edge_id(self, edge_id):
        done = bool(self.L.fwgpu_disconnect_edge(self.c, edge_id))
        if done:
            self._edges = {k: v for k, v in self._edges.items() if v[2] != edge_id}
        return done

    # ---- latency (include/fwgpu.h "latency compensation"): host-side queries over the current edges, no update() needed first
    def node_latency(self, node_id):
        """frames the node itself adds: 63 for a LimiterNode, `frames` for a DelayCompNode, 0 for every other kind"""
        n = C.c_uint32(0)
        self._check(self.L.fwgpu_node_latency(self.c, node_id, C.byref(n)))
        return n.value

    def latency_report(self):
        """[(node, input port, lead_frames)]: every connected input that the other inputs of its node are later than, by node, then port
        (fwgpu_graph_latency_report).  Raises CompileGraphError for a cyclic edge set, as update() would."""
        n = self.L.fwgpu_graph_latency_report(self.c, None, 0)
        buf = (_lib.LatencySkew * max(n, 1))()
        if n > 0:
            n = self.L.fwgpu_graph_latency_report(self.c, buf, n)
        if n in _COMPILE:
            raise CompileGraphError(n, self.L.fwgpu_last_error(self.c).decode())
        self._check(n)
        return [(buf[i].node, buf[i].port, buf[i].lead_frames) for i in range(n)]

    def output_latency(self):
        """frames the graph output is late by: the arrival latency at graph_out, the latest of its ports"""
        n = C.c_uint32(0)
        r = self.L.fwgpu_graph_output_latency(self.c, C.byref(n))
        if r in _COMPILE:
            raise CompileGraphError(r, self.L.fwgpu_last_error(self.c).decode())
        self._check(r)
        return n.value

    def compensate_latency(self):
        """Put a DelayCompNode of `lead_frames` on every edge latency_report names, so that all inputs of every node arrive together.
        Reported edges that share source node, destination node and lead go through one node of up to 8 channels.  Returns the ids
        of the nodes added (none when nothing is skewed: a second call adds none); the output latency stays what it was.  Edits the
        graph only: call update() afterwards.  Knows the edges made through this object's connect()."""
        groups = {}
        for node, port, lead in self.latency_report():
            if (node, port) not in self._edges:
                raise FwgpuError(-20, "compensate_latency: input %d of node %d was not connected through this context object" % (port, node))
            src, sport, _ = self._edges[(node, port)]
            groups.setdefault((src, node, lead), []).append((sport, port))
        added = []
        for (src, dst, lead), ports in groups.items():
            for i in range(0, len(ports), 8):
                chunk = ports[i:i + 8]
                prev = [(src, sport) for sport, _ in chunk]
                for sport, dport in chunk:
                    self.disconnect(src, sport, dst, dport)
                left = lead
                while left > 0:  # (a lead beyond one node's range: nodes in series)
                    d = min(left, DelayCompNode.MAX_FRAMES)
                    nid = self.add_node(len(chunk), len(chunk), DelayCompNode(d, channels=len(chunk)))
                    for k, (pn, pp) in enumerate(prev):
                        self.connect(pn, pp, nid, k)
                    prev = [(nid, k) for k in range(len(chunk))]
                    added.append(nid)
                    left -= d
                for (pn, pp), (_, dport) in zip(prev, chunk):
                    self.connect(pn, pp, dst, dport)
        return added

    def cycle_detected(self):
        return bool(self.L.fwgpu_cycle_detected(self.c))

    # ---- FirewheelGraphCtx::update (graph/context.rs:93-137)
    def update(self):
        r = self.L.fwgpu_update(self.c)
        if r in _COMPILE:
            raise CompileGraphError(r, self.L.fwgpu_last_error(self.c).decode())
        self._check(r)
        self._reap_limbo(updated=True)

    def plan_pending(self):
        """True while a plan built by update() / schedule_upload() waits for a process call to adopt it (include/fwgpu.h)"""
        return bool(self._check(self.L.fwgpu_plan_pending(self.c)))

    def schedule_upload(self, sched, num_buffers):
        """sched: list of dicts {"id", "in": [(buffer_index, should_clear)], "out": [buffer_index]} in schedule order
        (the reference's CompiledSchedule, schedule.rs:12-30)."""
        arr = (_lib.SchedNode * len(sched))()
        keep = []
        for i, s in enumerate(sched):
            ib = (C.c_uint32 * max(len(s["in"]), 1))(*[b for b, _ in s["in"]])
            ic = (C.c_uint8 * max(len(s["in"]), 1))(*[1 if c else 0 for _, c in s["in"]])
            ob = (C.c_uint32 * max(len(s["out"]), 1))(*s["out"])
            keep += [ib, ic, ob]
            arr[i].node = s["id"]
            arr[i].num_inputs = len(s["in"])
            arr[i].num_outputs = len(s["out"])
            arr[i].in_buffer_index = ib
            arr[i].in_should_clear = ic
            arr[i].out_buffer_index = ob
        r = self.L.fwgpu_schedule_upload(self.c, arr, len(sched), num_buffers)
        if r in _COMPILE:
            raise CompileGraphError(r, self.L.fwgpu_last_error(self.c).decode())
        self._check(r)
        self._reap_limbo(updated=True)

    # ---- plan introspection
    def plan_kind(self):
        return self.L.fwgpu_plan_kind(self.c)

    def plan_fused_voices(self):
        """voices of the installed plan that the fused kernels render (plan 3: the banks')"""
        return self.L.fwgpu_plan_fused_voices(self.c)

    def plan_num_levels(self):
        return self.L.fwgpu_plan_num_levels(self.c)

    def plan_node_level(self, node_id):
        return self.L.fwgpu_plan_node_level(self.c, node_id)

    def plan_node_inputs_clear(self, node_id):
        buf = (C.c_int * 64)()
        n = self._check(self.L.fwgpu_plan_node_inputs_clear(self.c, node_id, buf, 64))
        return [bool(buf[i]) for i in range(n)]

    def rt_resident_stats(self):
        """(resident realtime kernels launched, callbacks served through the doorbell) — include/fwgpu.h"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fwgpu_rt_resident_stats(self.c, C.byref(a), C.byref(b)))
        return a.value, b.value

    def rt_path_stats(self):
        """one-block launch batches by path: (resident kernel, one k_rt_block launch, the fused plans' launch sequence, the level
        executor) — include/fwgpu.h fwgpu_rt_path_stats"""
        a = (C.c_uint64 * 4)()
        self._check(self.L.fwgpu_rt_path_stats(self.c, a))
        return tuple(int(x) for x in a)

    def hip_stream(self):
        """the hipStream_t (int) the ctx's process calls launch on — include/fwgpu.h fwgpu_hip_stream"""
        return int(self.L.fwgpu_hip_stream(self.c) or 0)

    def fir_morph_stats(self):
        """(GEMM workgroups of FIR morph groups that ran, that returned idle) — include/fwgpu.h fwgpu_fir_morph_stats"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fwgpu_fir_morph_stats(self.c, C.byref(a), C.byref(b)))
        return a.value, b.value

    def lazy_stats(self):
        """(launch batches rendered without a control kernel, with one) — include/fwgpu.h fwgpu_lazy_stats"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fwgpu_lazy_stats(self.c, C.byref(a), C.byref(b)))
        return a.value, b.value

    def group_stats(self):
        """launch batches rendered by the one-pass kernel (leaves + root in one launch) — include/fwgpu.h fwgpu_plan_group_stats"""
        a = C.c_uint64(0)
        self._check(self.L.fwgpu_plan_group_stats(self.c, C.byref(a)))
        return a.value

    def plan_handover_stats(self):
        """(plans adopted so far, those adopted by a process call, the longest one of those held up its call in ns)"""
        a, b, m = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fwgpu_plan_handover_stats(self.c, C.byref(a), C.byref(b), C.byref(m)))
        return a.value, b.value, m.value

    def update_phase(self):
        """which part of fwgpu_update the control thread is in right now (0 none, 1 graph compile, 21..28 table sections, 3 the
        build's device work); any thread may ask"""
        return int(self.L.fwgpu_update_phase(self.c))

    def plan_chain_stats(self):
        """(steady, general): k_chain workgroup launches that ran the steady-call loop / the general loop"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fwgpu_plan_chain_stats(self.c, C.byref(a), C.byref(b)))
        return a.value, b.value

    def plan_host_nodes(self):
        """(host nodes in the installed plan, callbacks run since it was installed)"""
        n = C.c_uint64()
        return self._check(self.L.fwgpu_plan_host_nodes(self.c, C.byref(n))), n.value

    def set_max_batch(self, k):
        self._check(self.L.fwgpu_set_max_batch(self.c, k))

    def set_force_generic(self, on):
        self._check(self.L.fwgpu_set_force_generic(self.c, 1 if on else 0))

    # ---- SampleResource (core/sample_resource.rs)
    def new_sample(self, fmt, channels, data):
        a = np.ascontiguousarray(np.asarray(data, dtype=SampleFormat.DTYPE[fmt]))
        frames = a.size // channels
        return self._check(self.L.fwgpu_sample_create(self.c, fmt, channels, frames, a.ctypes.data_as(C.c_void_p)))

    def new_sample_device(self, fmt, channels, frames, device_ptr):
        return self._check(self.L.fwgpu_sample_create_device(self.c, fmt, channels, frames, C.c_void_p(device_ptr)))

    def new_stream(self, fmt, channels, ring_frames):
        """a StreamSource: a ring of `ring_frames` frames (4 * max_block_frames .. 2^30) that SamplerNode.set_sample accepts"""
        return StreamSource(self, fmt, channels, ring_frames)

    def destroy_sample(self, sample):
        """Release a sample's HBM (the last Arc<dyn SampleResource> dropped).  Refused while a FIR / resampler node
        names it; a sampler that still holds the id sees an empty sample from the next call on."""
        self._check(self.L.fwgpu_sample_destroy(self.c, sample))

    def poll_returned_samples(self, cap=64):
        """ProcessorToNodeMsg::ReturnSample (nodes/sampler.rs:339-343): [(node id, sample id)] a completed process call
        swapped out since the last poll — what SamplerNode::update() drains (sampler.rs:222-231)."""
        nodes, samples = (C.c_int64 * cap)(), (C.c_int * cap)()
        n = self._check(self.L.fwgpu_poll_returned_samples(self.c, nodes, samples, cap))
        return [(nodes[i], samples[i]) for i in range(n)]

    def sample_retired(self, sample):
        """True once no sampler holds the sample, no queued message names it and the device is done reading it."""
        return bool(self._check(self.L.fwgpu_sample_retired(self.c, sample)))

    def ext_pool_floats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fwgpu_ext_pool_floats(self.c, C.byref(a), C.byref(b)))
        return a.value, b.value

    def proc_info(self):
        """(stream_time_secs, stream_status, output_underflows, input_overflows) — ProcInfo of the last call (core/node.rs:111-132)"""
        t, st, u, o = C.c_double(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        self._check(self.L.fwgpu_proc_info(self.c, C.byref(t), C.byref(st), C.byref(u), C.byref(o)))
        return t.value, st.value, u.value, o.value

    def open_stream(self, num_in_channels=0, num_out_channels=2):
        return HeadlessStream(self, num_in_channels, num_out_channels)

    # ---- FirewheelProcessor::process_interleaved (graph/processor.rs:61-165)
    def process_interleaved(self, input, num_in_channels, num_out_channels, frames, stream_time_secs=0.0,
                            stream_status=0):
        out = np.full(frames * num_out_channels, np.nan, dtype=np.float32)
        if input is None:
            input = np.zeros(max(frames * num_in_channels, 1), dtype=np.float32)
        inp = np.ascontiguousarray(input, dtype=np.float32)
        self._check(self.L.fwgpu_process_interleaved(self.c, _fptr(inp), _fptr(out), num_in_channels, num_out_channels,
                                                     frames, stream_time_secs, stream_status))
        if self._limbo:  # (this call may have adopted the plan that no longer names a removed host node)
            self._reap_limbo()
        return out

    def process_interleaved_begin(self, input, num_in_channels, num_out_channels, frames, stream_time_secs=0.0, stream_status=0):
        """fwgpu_process_interleaved_begin: the call up to its last launch; returns the ticket `process_interleaved_end` takes"""
        if input is None:
            input = np.zeros(max(frames * num_in_channels, 1), dtype=np.float32)
        inp = np.ascontiguousarray(input, dtype=np.float32)
        t = self.L.fwgpu_process_interleaved_begin(self.c, _fptr(inp), num_in_channels, num_out_channels, frames, stream_time_secs, stream_status)
        self._check(t)
        return int(t), frames * num_out_channels

    def process_interleaved_end(self, ticket, out=None):
        """... and its other half: waits for the ticket's copy back, returns the frames (or fills `out`)"""
        t, n = ticket
        if out is None:
            out = np.full(n, np.nan, dtype=np.float32)
        self._check(self.L.fwgpu_process_interleaved_end(self.c, t, _fptr(out)))
        if self._limbo:
            self._reap_limbo()
        return out

    def process_interleaved_cancel(self, ticket):
        """abandon every ticket in flight up to and including this one (no frames copied)"""
        self._check(self.L.fwgpu_process_interleaved_cancel(self.c, ticket[0]))

    def process_blocks_device(self, num_blocks, device_out_ptr, num_out_channels=2):
        self._check(self.L.fwgpu_process_blocks_device(self.c, num_blocks, C.c_void_p(device_out_ptr), num_out_channels))

    def process_blocks_device_flags(self, num_blocks, device_out_ptr, num_out_channels, device_silence_ptr):
        """... also writing, per (block, channel), whether that graph-output channel was flagged silent (u8, device memory)"""
        self._check(self.L.fwgpu_process_blocks_device_flags(self.c, num_blocks, C.c_void_p(device_out_ptr), num_out_channels,
                                                             C.c_void_p(device_silence_ptr) if device_silence_ptr else None))

    def process_blocks_device_io(self, num_blocks, device_in_ptr, num_in_channels, device_out_ptr, num_out_channels=2, device_silence_ptr=None):
        """... for graphs with stream inputs: interleaved input frames in device memory (fwgpu_process_blocks_device_io)"""
        self._check(self.L.fwgpu_process_blocks_device_io(self.c, num_blocks, C.c_void_p(device_in_ptr) if device_in_ptr else None, num_in_channels,
                                                          C.c_void_p(device_out_ptr), num_out_channels,
                                                          C.c_void_p(device_silence_ptr) if device_silence_ptr else None))

    def bus_sum_ordered(self, part_ptrs, out_ptr, n_floats, silence_ptrs=None, out_silence_ptr=None, frames_per_block=0, n_channels=2):
        """the top-level R-port SumNode over the shards' partial buses (device pointers), rank order, on the ctx stream;
        silence_ptrs: per part, its [blocks][channels] silence flags as process_blocks_device_flags wrote them (sum.rs:122-124)"""
        arr = (C.c_void_p * len(part_ptrs))(*[C.c_void_p(p) for p in part_ptrs])
        if silence_ptrs is None:
            self._check(self.L.fwgpu_bus_sum_ordered(self.c, arr, len(part_ptrs), C.c_void_p(out_ptr), n_floats))
            return
        sil = (C.c_void_p * len(part_ptrs))(*[C.c_void_p(p) if p else None for p in silence_ptrs])
        self._check(self.L.fwgpu_bus_sum_ordered_flags(self.c, arr, sil, len(part_ptrs), C.c_void_p(out_ptr),
                                                       C.c_void_p(out_silence_ptr) if out_silence_ptr else None, n_floats,
                                                       frames_per_block, n_channels))

    def open_bus_exchange(self, rank, world, max_floats, max_silence_bytes=0):
        return BusExchange(self, rank, world, max_floats, max_silence_bytes)

    def synchronize(self):
        self._check(self.L.fwgpu_synchronize(self.c))

    def meter_read(self, node_id, first_block, num_blocks):
        """fwgpu_meter_read: (readings, blocks_done) — readings is a structured array [n][n_in] (METER_DTYPE: peak, sum_squares,
        over, frames) of the blocks [first_block, first_block + n) that exist yet, n <= num_blocks; blocks_done is the ctx's block
        count.  Waits for the ctx stream.  Raises FwgpuError (-20) for a node that is no meter of the installed plan and for blocks
        the ring no longer holds; the error carries the block count as `blocks_done`."""
        n_in = 0
        node = self._nodes.get(node_id)
        if node is not None:
            n_in = getattr(node, "_n_in", 0)
        buf = np.zeros((max(num_blocks, 1), max(n_in, 1)), dtype=METER_DTYPE)
        done = C.c_uint64(0)
        n = self.L.fwgpu_meter_read(self.c, node_id, first_block, num_blocks, buf.ctypes.data_as(C.POINTER(_lib.MeterReading)) if num_blocks and n_in else None,
                                    C.byref(done))
        if n < 0:
            e = FwgpuError(n, self.L.fwgpu_last_error(self.c).decode())
            e.blocks_done = done.value
            raise e
        return buf[:n, :n_in], done.value

    def spectrum_layout(self, node_id):
        """fwgpu_spectrum_layout: (fft_size, bands, edges) of a spectrum meter of the installed plan — `bands` as created (0: every bin),
        edges a uint32 array of B + 1 entries, B the floats of one record.  Raises FwgpuError (-20) for any other node"""
        n, b = C.c_uint32(0), C.c_uint32(0)
        B = self.L.fwgpu_spectrum_layout(self.c, node_id, C.byref(n), C.byref(b), None, 0)
        if B < 0:
            raise FwgpuError(B, self.L.fwgpu_last_error(self.c).decode())
        edges = np.zeros(B + 1, dtype=np.uint32)
        self._check(min(0, self.L.fwgpu_spectrum_layout(self.c, node_id, None, None, edges.ctypes.data_as(C.POINTER(C.c_uint32)), B + 1)))
        return n.value, b.value, edges

    def spectrum_read(self, node_id, first_block, num_blocks):
        """fwgpu_spectrum_read: (powers, blocks_done) — powers is a float32 array [n][n_in][B] of the blocks [first_block, first_block
        + n) that exist yet, with fwgpu_meter_read's rules and errors (a plain meter: -20)"""
        node = self._nodes.get(node_id)
        n_in = getattr(node, "_n_in", 0) if node is not None else 0
        done = C.c_uint64(0)
        B = self.L.fwgpu_spectrum_layout(self.c, node_id, None, None, None, 0)
        if B < 0:
            n = self.L.fwgpu_spectrum_read(self.c, node_id, first_block, 0, None, C.byref(done))  # (for the block count and the message)
            e = FwgpuError(n if n < 0 else B, self.L.fwgpu_last_error(self.c).decode())
            e.blocks_done = done.value
            raise e
        buf = np.zeros((max(num_blocks, 1), max(n_in, 1), B), dtype=np.float32)
        n = self.L.fwgpu_spectrum_read(self.c, node_id, first_block, num_blocks, buf.ctypes.data_as(C.POINTER(C.c_float)) if num_blocks and n_in else None,
                                       C.byref(done))
        if n < 0:
            e = FwgpuError(n, self.L.fwgpu_last_error(self.c).decode())
            e.blocks_done = done.value
            raise e
        return buf[:n, :n_in], done.value

    # ---- AudioNodeProcessor::process for one node on host buffers (core/node.rs:37-53)
    def node_process(self, node_id, frames, inputs, outputs, in_silence_mask=0, out_silence_mask=0):
        ins = [np.ascontiguousarray(x, dtype=np.float32) for x in inputs]
        for o in outputs:
            assert o.dtype == np.float32 and o.flags["C_CONTIGUOUS"]
        it = (C.POINTER(C.c_float) * max(len(ins), 1))(*[_fptr(a) for a in ins])
        ot = (C.POINTER(C.c_float) * max(len(outputs), 1))(*[_fptr(a) for a in outputs])
        om = C.c_uint64(out_silence_mask)
        self._check(self.L.fwgpu_node_process(self.c, node_id, frames, it, len(ins), ot, len(outputs), in_silence_mask,
                                              C.byref(om), 0.0, 0))
        return om.value

    # ---- measurement hooks
    def timing_enable(self, on=True):
        self._check(self.L.fwgpu_timing_enable(self.c, 1 if on else 0))

    def timing_read(self, which=0):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.L.fwgpu_timing_read(self.c, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timing_reset(self):
        self._check(self.L.fwgpu_timing_reset(self.c))

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, hbm = C.c_int(), C.c_uint64()
        self._check(self.L.fwgpu_device_info(self.c, name, 256, C.byref(cus), C.byref(hbm)))
        return name.value.decode(), cus.value, hbm.value


class BusExchange(object):
    """The multi-GPU mix bus behind the C ABI (fwgpu_bus_exchange_*, SURVEY §8e path 2): every rank stores its partial bus
    into its slot on every rank (peer-mapped over xGMI, or by pointer inside one process), then adds the R slots it holds in
    rank order — the top-level R-port SumNode (nodes/sum.rs:41-136), bit-identical to the single-process graph."""

    def __init__(self, cx, rank, world, max_floats, max_silence_bytes=0):
        self.cx, self.rank, self.world = cx, rank, world
        self.x = cx.L.fwgpu_bus_exchange_open(cx.c, rank, world, max_floats, max_silence_bytes)
        if not self.x:
            raise FwgpuError(-30, cx.L.fwgpu_last_error(cx.c).decode())

    def export(self):
        """this rank's handle (bytes) — carry it to the peers through any side channel"""
        buf = C.create_string_buffer(_lib.EXCHANGE_HANDLE_BYTES)
        self.cx._check(self.cx.L.fwgpu_bus_exchange_export(self.x, buf))
        return buf.raw

    def connect(self, peer_rank, handle):
        buf = C.create_string_buffer(bytes(handle), _lib.EXCHANGE_HANDLE_BYTES)
        self.cx._check(self.cx.L.fwgpu_bus_exchange_connect(self.x, peer_rank, buf))

    def connect_all(self, handles):
        for r, h in enumerate(handles):
            if r != self.rank:
                self.connect(r, h)

    def set_timeout_ms(self, ms):
        self.cx._check(self.cx.L.fwgpu_bus_exchange_set_timeout_ms(self.x, ms))

    def push(self, part_ptr, n_floats, silence_ptr=None, n_blocks=0, n_channels=2):
        self.cx._check(self.cx.L.fwgpu_bus_exchange_push(self.x, C.c_void_p(part_ptr), C.c_void_p(silence_ptr) if silence_ptr else None,
                                                         n_floats, n_blocks, n_channels))

    def reduce(self, out_ptr, n_floats, out_silence_ptr=None, n_blocks=0, frames_per_block=0, n_channels=2, have_silence=False):
        self.cx._check(self.cx.L.fwgpu_bus_exchange_reduce(self.x, C.c_void_p(out_ptr), C.c_void_p(out_silence_ptr) if out_silence_ptr else None,
                                                           n_floats, n_blocks, frames_per_block, n_channels, 1 if have_silence else 0))

    def step(self, part_ptr, out_ptr, n_floats, silence_ptr=None, out_silence_ptr=None, n_blocks=0, frames_per_block=0, n_channels=2):
        self.cx._check(self.cx.L.fwgpu_bus_exchange_step(self.x, C.c_void_p(part_ptr), C.c_void_p(silence_ptr) if silence_ptr else None,
                                                         C.c_void_p(out_ptr), C.c_void_p(out_silence_ptr) if out_silence_ptr else None,
                                                         n_floats, n_blocks, frames_per_block, n_channels))

    def status(self):
        """(reduces issued, 0 or the first step a peer did not arrive for) — waits for the ctx stream; raises on a failed step"""
        a, b = C.c_uint64(), C.c_uint64()
        rc = self.cx.L.fwgpu_bus_exchange_status(self.x, C.byref(a), C.byref(b))
        if rc < 0:
            raise FwgpuError(rc, "%s (step %d)" % (self.cx.L.fwgpu_last_error(self.cx.c).decode(), b.value))
        return a.value, b.value

    def wait_stats(self, reset=False):
        """[us] the longest a reduce of this rank has waited for each rank's arrival so far (waits for the ctx stream)"""
        buf = (C.c_uint64 * self.world)()
        self.cx._check(self.cx.L.fwgpu_bus_exchange_wait_stats(self.x, buf, self.world, 1 if reset else 0))
        return [int(v) for v in buf]

    def close(self):
        if getattr(self, "x", None) and getattr(self.cx, "c", None):
            self.cx.L.fwgpu_bus_exchange_close(self.x)
        self.x = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HeadlessStream(object):
    """DataCallback (firewheel-cpal/src/lib.rs:362-449) without a device: `callback(frames, instant)` once per device
    period, `instant` = the backend's clock at that callback in seconds (cpal: info.timestamp().callback)."""

    OUTPUT_UNDERFLOW = 2  # StreamStatus (core/node.rs:120-132)
    INPUT_OVERFLOW = 1

    def __init__(self, cx, num_in_channels, num_out_channels):
        self.cx = cx
        self.num_out_channels = num_out_channels
        self.s = cx.L.fwgpu_stream_open(cx.c, num_in_channels, num_out_channels)
        if not self.s:
            raise FwgpuError(-20, "fwgpu_stream_open failed")

    def callback(self, frames, instant_secs):
        """returns (interleaved output, StreamStatus bits handed to process_interleaved)"""
        out = np.full(frames * self.num_out_channels, np.nan, dtype=np.float32)
        st = self.cx._check(self.cx.L.fwgpu_stream_callback(self.s, _fptr(out), frames, instant_secs))
        return out, st

    def run(self, frames, n_callbacks, first_instant_secs=0.0):
        """the backend thread's loop (fwgpu_stream_run): n callbacks back to back inside the library.  Returns (the last
        block, seconds the loop took)"""
        out = np.full(frames * self.num_out_channels, np.nan, dtype=np.float32)
        dt = C.c_double()
        self.cx._check(self.cx.L.fwgpu_stream_run(self.s, _fptr(out), frames, n_callbacks, first_instant_secs, C.byref(dt)))
        return out, dt.value

    def stats(self):
        a, b, t = C.c_uint64(), C.c_uint64(), C.c_double()
        self.cx._check(self.cx.L.fwgpu_stream_stats(self.s, C.byref(a), C.byref(b), C.byref(t)))
        return a.value, b.value, t.value

    def close(self):
        if self.s:
            self.cx.L.fwgpu_stream_close(self.s)
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
