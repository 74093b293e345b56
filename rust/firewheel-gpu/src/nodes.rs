//! Level B1: Firewheel's built-in nodes (firewheel-graph/src/basic_nodes/*.rs) — and the north-star nodes the reference
//! lists as TODO (README.md:14-19) — as `AudioNode`s whose processor half runs on the device.
//!
//! Each wrapper has the reference node's constructor and control-half setters.  `activate()` registers the node with
//! the shared [`GpuContext`] (`fwgpu_add_node` + `fwgpu_update`) — on Firewheel's control thread, WHILE the audio thread may
//! be inside `process()` of nodes that are already active (graph.rs:586-612): libfwgpu builds the new plan off to the side
//! and the audio thread's next `fwgpu_node_process` adopts it, and that call looks the node up in the ACTIVE plan, never in
//! the graph being edited — and returns a [`GpuNodeProcessor`], whose `process()`
//! is one `fwgpu_node_process` call: the same device function the whole-graph executor runs for that node, on the
//! caller's buffers, with `in_silence_mask` / `out_silence_mask` honoured (core/node.rs:94-118).  Setters become
//! messages (`fwgpu_node_set_param`, `fwgpu_sampler_*`) with `at_block = 0`: a per-block caller gets the reference's
//! "polled at the top of process()" semantics exactly (volume.rs:92, sampler.rs:331).
use std::error::Error;
use std::sync::Arc;

use arrayvec::ArrayVec;
use firewheel_core::node::{AudioNode, AudioNodeInfo, AudioNodeProcessor, ProcInfo};
use firewheel_core::SilenceMask;

use crate::sample::GpuSample;
use crate::{ffi, GpuContext, GpuError};

/// `AudioNodeProcessor` of every GPU node: forwards the block to `fwgpu_node_process`.
pub struct GpuNodeProcessor {
    cx: Arc<GpuContext>,
    node: i64,
}
impl AudioNodeProcessor for GpuNodeProcessor {
    fn process(&mut self, frames: usize, inputs: &[&[f32]], outputs: &mut [&mut [f32]], proc_info: ProcInfo) {
        let ins: ArrayVec<*const f32, 64> = inputs.iter().map(|s| s.as_ptr()).collect();
        let outs: ArrayVec<*mut f32, 64> = outputs.iter_mut().map(|s| s.as_mut_ptr()).collect();
        let mut out_mask: u64 = proc_info.out_silence_mask.0; // 0 on entry (graph/processor.rs:233)
        let rc = unsafe {
            ffi::fwgpu_node_process(
                self.cx.as_ptr(),
                self.node,
                frames as u64,
                ins.as_ptr(),
                ins.len() as u32,
                outs.as_ptr(),
                outs.len() as u32,
                proc_info.in_silence_mask.0,
                &mut out_mask,
                proc_info.stream_time_secs,
                proc_info.stream_status.bits(),
            )
        };
        if rc < 0 {
            // "all output buffers MUST be filled" (core/node.rs:41-42)
            firewheel_core::util::clear_all_outputs(frames, outputs, proc_info.out_silence_mask);
            return;
        }
        *proc_info.out_silence_mask = SilenceMask(out_mask);
    }
}

/// What every wrapper shares: the context, the device node id once activated.
struct Binding {
    cx: Arc<GpuContext>,
    node: Option<i64>,
}
impl Binding {
    fn new(cx: &Arc<GpuContext>) -> Self {
        Self { cx: Arc::clone(cx), node: None }
    }
    fn activate(
        &mut self,
        kind: i32,
        num_inputs: usize,
        num_outputs: usize,
        params: &[f32],
    ) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        let node = self.cx.add_node(kind, num_inputs as u32, num_outputs as u32, params)?;
        // activation checks (volume.rs:63-65, sum.rs:27-29, hard_clip.rs:37-39) run in fwgpu_update and come back as
        // FWGPU_ERR_NODE_ACTIVATION_FAILED + the reference's message
        if let Err(e) = self.cx.update() {
            let _ = self.cx.remove_node(node);
            return Err(Box::new(e));
        }
        self.node = Some(node);
        Ok(Box::new(GpuNodeProcessor { cx: Arc::clone(&self.cx), node }))
    }
    fn deactivate(&mut self) {
        if let Some(node) = self.node.take() {
            let _ = self.cx.remove_node(node);
        }
    }
    fn set_param(&self, param: i32, value: f32) -> Result<(), GpuError> {
        match self.node {
            Some(node) => {
                let _g = self.cx.control();
                self.cx.check(unsafe { ffi::fwgpu_node_set_param(self.cx.as_ptr(), node, param, value, 0) } as i64).map(|_| ())
            }
            None => Ok(()), // not activated yet: the constructor argument carries the value (activate reads it)
        }
    }
}

fn io(min_in: u32, max_in: u32, min_out: u32, max_out: u32, updates: bool) -> AudioNodeInfo {
    AudioNodeInfo {
        num_min_supported_inputs: min_in,
        num_max_supported_inputs: max_in,
        num_min_supported_outputs: min_out,
        num_max_supported_outputs: max_out,
        updates,
    }
}

// ------------------------------------------------------------------------------------------------ VolumeNode
/// basic_nodes/volume.rs:8-77
pub struct GpuVolumeNode {
    b: Binding,
    percent_volume: f32,
}
impl GpuVolumeNode {
    pub fn new(cx: &Arc<GpuContext>, percent_volume: f32) -> Self {
        Self { b: Binding::new(cx), percent_volume: percent_volume.max(0.0) }
    }
    pub fn percent_volume(&self) -> f32 {
        self.percent_volume
    }
    /// volume.rs:28-34 — the `Arc<AtomicF32>` store becomes a message in libfwgpu's lock-free ring
    pub fn set_percent_volume(&mut self, percent_volume: f32) {
        self.percent_volume = percent_volume.max(0.0);
        let _ = self.b.set_param(0, percent_volume);
    }
    /// the longest ride one message takes, in frames
    pub const RIDE_FRAMES_MAX: u32 = ffi::FWGPU_GAIN_RIDE_FRAMES_MAX;
    /// From the next block on, ride the gain from where it stands to what `percent_volume` sets, over `frames` frames (0: a hard set
    /// with no 10 ms glide) along `curve` — one message instead of a `set_percent_volume` per block.  A second ride starts where the
    /// first stands; `set_percent_volume` during a ride ends it and glides on from its current value.  Before activation only the
    /// target is kept: the node then starts there.
    pub fn ride_to(&mut self, percent_volume: f32, frames: u32, curve: CrossfadeCurve) -> Result<(), GpuError> {
        gain_ride(&self.b, percent_volume, frames, curve)?;
        self.percent_volume = percent_volume.max(0.0);
        Ok(())
    }
    /// ... over `secs` seconds, rounded to whole frames of `sample_rate`
    pub fn ride_to_secs(&mut self, percent_volume: f32, secs: f64, sample_rate: u32, curve: CrossfadeCurve) -> Result<(), GpuError> {
        self.ride_to(percent_volume, (secs * sample_rate as f64).round().max(0.0) as u32, curve)
    }
}
/// fwgpu_gain_ride for a volume or a pan node that is active (before activation there is nothing to send)
fn gain_ride(b: &Binding, value: f32, frames: u32, curve: CrossfadeCurve) -> Result<(), GpuError> {
    let (shape, x1, y1, x2, y2) = match curve {
        CrossfadeCurve::Linear => (0, 0.0, 0.0, 1.0, 1.0),
        CrossfadeCurve::Bezier(x1, y1, x2, y2) => (1, x1, y1, x2, y2),
    };
    if let Some(node) = b.node {
        let _g = b.cx.control();
        let rc = unsafe { ffi::fwgpu_gain_ride(b.cx.as_ptr(), node, value, frames, shape, x1, y1, x2, y2, 0) };
        b.cx.check(rc as i64)?;
    }
    Ok(())
}
impl AudioNode for GpuVolumeNode {
    fn debug_name(&self) -> &'static str {
        "volume"
    }
    fn info(&self) -> AudioNodeInfo {
        io(1, 64, 1, 64, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(ffi::FWGPU_VOLUME, num_inputs, num_outputs, &[self.percent_volume])
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

// ------------------------------------------------------------------------------------------------ SumNode
/// basic_nodes/sum.rs:3-35
pub struct GpuSumNode {
    b: Binding,
}
impl GpuSumNode {
    pub fn new(cx: &Arc<GpuContext>) -> Self {
        Self { b: Binding::new(cx) }
    }
}
impl AudioNode for GpuSumNode {
    fn debug_name(&self) -> &'static str {
        "sum"
    }
    fn info(&self) -> AudioNodeInfo {
        io(1, 64, 1, 64, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(ffi::FWGPU_SUM, num_inputs, num_outputs, &[])
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

// ------------------------------------------------------------------------------------------------ SamplerNode
/// basic_nodes/sampler.rs:16-19
#[derive(Debug, Clone, PartialEq)]
pub enum LoopRange {
    Full,
    RangeSecs(std::ops::Range<f64>),
}

/// basic_nodes/sampler.rs:46-233.  `set_sample` takes a [`GpuSample`] (the device-resident counterpart of
/// `S: SampleResource`); the sample the processor hands back (`ReturnSample`, :339-343) is dropped in `update()`.
pub struct GpuSamplerNode {
    b: Binding,
    percent_volume: f32,
    playing: bool,
    held: Vec<GpuSample>, // handles the device may still be reading: released when it hands the id back
}
impl GpuSamplerNode {
    pub fn new(cx: &Arc<GpuContext>, percent_volume: f32) -> Self {
        Self { b: Binding::new(cx), percent_volume: percent_volume.max(0.0), playing: false, held: Vec::new() }
    }
    fn msg(&self, f: impl FnOnce(*mut ffi::fwgpu_ctx, i64) -> i32) -> Result<(), ()> {
        let node = self.b.node.ok_or(())?; // not activated: sampler.rs:68-70 returns Err(())
        let _g = self.b.cx.control();
        if f(self.b.cx.as_ptr(), node) < 0 {
            return Err(()); // ring full (FWGPU_ERR_QUEUE_FULL): sampler.rs:72-78 `.map_err(|_| ())`
        }
        Ok(())
    }
    /// sampler.rs:67-79
    pub fn set_sample(&mut self, sample: GpuSample, stop_playback: bool) -> Result<(), ()> {
        let id = sample.id();
        self.msg(|c, n| unsafe { ffi::fwgpu_sampler_set_sample(c, n, id, stop_playback as i32, 0) })?;
        self.held.push(sample);
        if stop_playback {
            self.playing = false;
        }
        Ok(())
    }
    /// sampler.rs:82-97
    pub fn play(&mut self) -> Result<(), ()> {
        self.msg(|c, n| unsafe { ffi::fwgpu_sampler_play(c, n, 0) })?;
        self.playing = true;
        Ok(())
    }
    /// sampler.rs:100-115
    pub fn pause(&mut self) -> Result<(), ()> {
        self.msg(|c, n| unsafe { ffi::fwgpu_sampler_pause(c, n, 0) })?;
        self.playing = false;
        Ok(())
    }
    /// sampler.rs:118-133
    pub fn stop(&mut self) -> Result<(), ()> {
        self.msg(|c, n| unsafe { ffi::fwgpu_sampler_stop(c, n, 0) })?;
        self.playing = false;
        Ok(())
    }
    /// the longest fade one message takes, in frames
    pub const FADE_FRAMES_MAX: u32 = ffi::FWGPU_SAMPLER_FADE_FRAMES_MAX;
    /// SPEC gain envelope: from the next block on, move the voice's envelope to `gain` (0..1) over `frames`
    /// frames, linearly (0: a step), and at the fade's end do `then` (`ffi::FWGPU_FADE_NONE`, `_PAUSE` or `_STOP`) — a declicked
    /// pause or stop in one message.  The envelope is a transient: every pause and stop puts it back to 1.0, so a level that should
    /// last belongs in `percent_volume`.  With a `then`, `playing` is false from this call on, as after `pause` / `stop`.
    pub fn fade_to(&mut self, gain: f32, frames: u32, then: i32) -> Result<(), ()> {
        self.msg(|c, n| unsafe { ffi::fwgpu_sampler_fade(c, n, gain, frames, then, 0) })?;
        if then != ffi::FWGPU_FADE_NONE {
            self.playing = false;
        }
        Ok(())
    }
    /// a declicked start of a voice that is not playing: the envelope steps to 0, the voice plays, the envelope rises to 1 over `frames`
    pub fn fade_in(&mut self, frames: u32) -> Result<(), ()> {
        self.fade_to(0.0, 0, ffi::FWGPU_FADE_NONE)?;
        self.play()?;
        self.fade_to(1.0, frames, ffi::FWGPU_FADE_NONE)
    }
    /// sampler.rs:136-147
    pub fn set_playhead(&mut self, playhead_secs: f64) -> Result<(), ()> {
        self.msg(|c, n| unsafe { ffi::fwgpu_sampler_set_playhead_secs(c, n, playhead_secs, 0) })
    }
    /// sampler.rs:150-161
    pub fn set_loop_range(&mut self, loop_range: Option<LoopRange>) -> Result<(), ()> {
        let (mode, s, e) = match loop_range {
            None => (0, 0.0, 0.0),
            Some(LoopRange::Full) => (1, 0.0, 0.0),
            Some(LoopRange::RangeSecs(r)) => (2, r.start, r.end),
        };
        self.msg(|c, n| unsafe { ffi::fwgpu_sampler_set_loop_range(c, n, mode, s, e, 0) })
    }
    pub fn is_playing(&self) -> bool {
        self.playing
    }
    pub fn percent_volume(&self) -> f32 {
        self.percent_volume
    }
    /// sampler.rs:171-177
    pub fn set_percent_volume(&mut self, percent_volume: f32) {
        self.percent_volume = percent_volume.max(0.0);
        let _ = self.b.set_param(0, percent_volume);
    }
}
/// What [`GpuStreamSource::status`] reports, as of the last completed process call.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct StreamStatus {
    /// frames of data accepted so far (the end's padding not counted)
    pub written: u64,
    /// frames the sampler has played
    pub consumed: u64,
    /// blocks that were silent because their frames were not in the ring yet
    pub starved_blocks: u64,
    /// the sampler has played past the end, or has let go of the stream
    pub finished: bool,
}

/// SPEC streaming source (include/fwgpu.h `fwgpu_sample_create_stream`): a sample whose storage is a ring of
/// `ring_frames` frames (4 x max_block_frames ..= 2^30) that the control side appends to while ONE sampler plays it — a music track
/// that sounds before it is decoded to its end, a voice chat, a radio.  Hand it to [`GpuSamplerNode::set_stream`] once; `write` what the
/// decoder produces whenever there is room, `end` behind the last frame.  A block whose frames are not there yet is silent and the
/// voice carries on in the block in which they are.
pub struct GpuStreamSource {
    cx: Arc<GpuContext>,
    sample: GpuSample,
    channels: u32,
    elem_bytes: usize,
    ended: bool,
}
impl GpuStreamSource {
    pub fn new(cx: &Arc<GpuContext>, graveyard: &Arc<crate::sample::Graveyard>, format: i32, channels: u32, ring_frames: u64) -> Result<Self, GpuError> {
        let sample = GpuSample::create_stream(cx, graveyard, format, channels, ring_frames)?;
        let elem_bytes = if format == ffi::FWGPU_INTERLEAVED_F32 || format == ffi::FWGPU_PLANAR_F32 { 4 } else { 2 };
        Ok(Self { cx: Arc::clone(cx), sample, channels, elem_bytes, ended: false })
    }
    pub fn sample(&self) -> &GpuSample {
        &self.sample
    }
    /// Append frames: `data` holds whole frames of the stream's format, laid out as a sample of that many frames (planar: channel c
    /// starts c x frames elements in).  Returns the frames accepted, 0..=frames — the ring's free space as of the last process call
    /// known to be complete; `Err` with `FWGPU_ERR_QUEUE_FULL` when the sampler's message ring is full (repeat the call).
    pub fn write(&mut self, data: &[u8]) -> Result<u64, GpuError> {
        let frames = (data.len() / (self.elem_bytes * self.channels as usize)) as u64;
        let _g = self.cx.control();
        let rc = unsafe { ffi::fwgpu_sample_stream_write(self.cx.as_ptr(), self.sample.id(), data.as_ptr().cast(), frames) };
        Ok(self.cx.check(rc as i64)? as u64)
    }
    /// No more data: the sampler stops behind the last frame written.  `Err` with `FWGPU_ERR_QUEUE_FULL` while the ring has no room
    /// for the padding yet (repeat the call after the next process call).
    pub fn end(&mut self) -> Result<(), GpuError> {
        let _g = self.cx.control();
        self.cx.check(unsafe { ffi::fwgpu_sample_stream_end(self.cx.as_ptr(), self.sample.id()) } as i64)?;
        self.ended = true;
        Ok(())
    }
    pub fn has_ended(&self) -> bool {
        self.ended
    }
    /// never blocks
    pub fn status(&self) -> Result<StreamStatus, GpuError> {
        let (mut w, mut c, mut u, mut f) = (0u64, 0u64, 0u64, 0i32);
        let _g = self.cx.control();
        self.cx.check(unsafe { ffi::fwgpu_sample_stream_status(self.cx.as_ptr(), self.sample.id(), &mut w, &mut c, &mut u, &mut f) } as i64)?;
        Ok(StreamStatus { written: w, consumed: c, starved_blocks: u, finished: f != 0 })
    }
}
impl GpuSamplerNode {
    /// bind a stream to this sampler — once per stream; seek and loop messages are refused while the sampler holds it
    pub fn set_stream(&mut self, stream: &GpuStreamSource, stop_playback: bool) -> Result<(), ()> {
        self.set_sample(stream.sample().clone(), stop_playback)
    }
}
impl AudioNode for GpuSamplerNode {
    fn debug_name(&self) -> &'static str {
        "sampler"
    }
    fn info(&self) -> AudioNodeInfo {
        io(0, 0, 1, 64, true) // sampler.rs:188-195: updates = true
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(ffi::FWGPU_SAMPLER, num_inputs, num_outputs, &[self.percent_volume])
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate();
        self.held.clear(); // the ids go to the graveyard; they are destroyed once fwgpu_sample_retired agrees
    }
    /// sampler.rs:222-231: drain `ReturnSample`.  The ring is per context in libfwgpu, so the owner of the context
    /// usually polls once and routes by node id; a single-sampler host can let the node do it.
    fn update(&mut self) {
        let Some(node) = self.b.node else { return };
        let mut nodes = [0i64; 16];
        let mut samples = [0i32; 16];
        let _g = self.b.cx.control();
        let n = unsafe { ffi::fwgpu_poll_returned_samples(self.b.cx.as_ptr(), nodes.as_mut_ptr(), samples.as_mut_ptr(), 16) };
        for i in 0..n.max(0) as usize {
            if nodes[i] == node {
                if let Some(pos) = self.held.iter().position(|s| s.id() == samples[i]) {
                    self.held.swap_remove(pos); // drop on the control thread, like `ReturnSample(_smp) => {}`
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ BeepTestNode
/// basic_nodes/beep_test.rs:8-62
pub struct GpuBeepTestNode {
    b: Binding,
    freq_hz: f32,
    gain_db: f32,
    enabled: bool,
}
impl GpuBeepTestNode {
    pub fn new(cx: &Arc<GpuContext>, freq_hz: f32, gain_db: f32, enabled: bool) -> Self {
        Self { b: Binding::new(cx), freq_hz, gain_db, enabled }
    }
    pub fn enabled(&self) -> bool {
        self.enabled
    }
    /// beep_test.rs:30-32
    pub fn set_enabled(&mut self, enabled: bool) {
        self.enabled = enabled;
        let _ = self.b.set_param(0, if enabled { 1.0 } else { 0.0 });
    }
}
impl AudioNode for GpuBeepTestNode {
    fn debug_name(&self) -> &'static str {
        "beep_test"
    }
    fn info(&self) -> AudioNodeInfo {
        io(0, 0, 1, 64, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        // the clamps of beep_test.rs:16-17 are applied by fwgpu_add_node
        self.b.activate(ffi::FWGPU_BEEP_TEST, num_inputs, num_outputs, &[self.freq_hz, self.gain_db, self.enabled as i32 as f32])
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

// ------------------------------------------------------------------------------------------------ parameterless / one-shot nodes
macro_rules! simple_node {
    ($name:ident, $debug:expr, $kind:expr, $info:expr, $doc:expr, [$($field:ident : $ty:ty),*]) => {
        #[doc = $doc]
        pub struct $name {
            b: Binding,
            $(pub $field: $ty,)*
        }
        impl $name {
            pub fn new(cx: &Arc<GpuContext> $(, $field: $ty)*) -> Self {
                Self { b: Binding::new(cx) $(, $field)* }
            }
        }
        impl AudioNode for $name {
            fn debug_name(&self) -> &'static str {
                $debug
            }
            fn info(&self) -> AudioNodeInfo {
                $info
            }
            fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
                self.b.activate($kind, num_inputs, num_outputs, &[$(self.$field as f32),*])
            }
            fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
                self.b.deactivate()
            }
        }
    };
}
simple_node!(GpuHardClipNode, "hard_clip", ffi::FWGPU_HARD_CLIP, io(1, 64, 1, 64, false), "basic_nodes/hard_clip.rs:3-41", [threshold_db: f32]);
simple_node!(GpuMonoToStereoNode, "mono_to_stereo", ffi::FWGPU_MONO_TO_STEREO, io(1, 1, 2, 2, false), "basic_nodes/mono_to_stereo.rs", []);
simple_node!(GpuStereoToMonoNode, "stereo_to_mono", ffi::FWGPU_STEREO_TO_MONO, io(2, 2, 1, 1, false), "basic_nodes/stereo_to_mono.rs", []);
simple_node!(GpuDummyNode, "dummy", ffi::FWGPU_DUMMY, io(0, 64, 0, 64, false), "basic_nodes/dummy.rs", []);

// ------------------------------------------------------------------------------------------------ north-star nodes (README.md:14-19; SPEC in the fwgpu repository's DESIGN.md §6)
macro_rules! param_node {
    ($name:ident, $debug:expr, $kind:expr, $info:expr, $doc:expr, [$($field:ident),*], {$($setter:ident => ($param:expr, $sfield:ident)),*}) => {
        #[doc = $doc]
        pub struct $name {
            b: Binding,
            $($field: f32,)*
        }
        impl $name {
            pub fn new(cx: &Arc<GpuContext> $(, $field: f32)*) -> Self {
                Self { b: Binding::new(cx) $(, $field)* }
            }
            $(pub fn $setter(&mut self, value: f32) {
                self.$sfield = value;
                let _ = self.b.set_param($param, value);
            })*
        }
        impl AudioNode for $name {
            fn debug_name(&self) -> &'static str {
                $debug
            }
            fn info(&self) -> AudioNodeInfo {
                $info
            }
            fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
                self.b.activate($kind, num_inputs, num_outputs, &[$(self.$field),*])
            }
            fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
                self.b.deactivate()
            }
        }
    };
}
param_node!(GpuStereoPanNode, "stereo_pan", ffi::FWGPU_STEREO_PAN, io(2, 2, 2, 2, false),
            "equal-power stereo pan, pan in [-1, 1], one ParamSmoother per channel", [pan], {set_pan => (0, pan)});
impl GpuStereoPanNode {
    /// the longest ride one message takes, in frames
    pub const RIDE_FRAMES_MAX: u32 = ffi::FWGPU_GAIN_RIDE_FRAMES_MAX;
    /// From the next block on, ride both ear gains from where they stand to what `pan` sets, over `frames` frames (0: a hard set) along
    /// `curve`.  The ride travels in the gains, each ear on its own: a ride from hard left to hard right dips in power at the middle —
    /// one that must hold power is two rides through the centre.  A setter during a ride ends it.
    pub fn ride_to(&mut self, pan: f32, frames: u32, curve: CrossfadeCurve) -> Result<(), GpuError> {
        gain_ride(&self.b, pan, frames, curve)?;
        self.pan = pan;
        Ok(())
    }
    /// ... over `secs` seconds, rounded to whole frames of `sample_rate`
    pub fn ride_to_secs(&mut self, pan: f32, secs: f64, sample_rate: u32, curve: CrossfadeCurve) -> Result<(), GpuError> {
        self.ride_to(pan, (secs * sample_rate as f64).round().max(0.0) as u32, curve)
    }
}
param_node!(GpuStereoWidthNode, "stereo_width", ffi::FWGPU_STEREO_WIDTH, io(2, 2, 2, 2, false),
            "mid/side width, one smoothed parameter (0 = mono, 1 = unchanged)", [width], {set_width => (0, width)});
param_node!(GpuBiquadNode, "biquad", ffi::FWGPU_BIQUAD, io(1, 64, 1, 64, false),
            "RBJ biquad (filter_type 0 = low-pass, 1 = high-pass, 2 = band-pass), Direct Form I in f32",
            [filter_type, cutoff_hz, q], {set_cutoff_hz => (1, cutoff_hz), set_q => (2, q)});
impl GpuBiquadNode {
    /// the longest sweep one message takes, in frames
    pub const SWEEP_FRAMES_MAX: u32 = ffi::FWGPU_BIQUAD_SWEEP_FRAMES_MAX;
    /// From the next block on, move the filter to (`cutoff_hz`, `q`) over `frames` frames: the five coefficients travel linearly and
    /// per frame (0: a step, as `set_cutoff_hz`) — one message for an occlusion or under-water muffle.  A second sweep starts from
    /// where the first stands.  Before activation only the target is kept: the node then starts there.  The node's recorded cutoff
    /// and Q are the TARGET from this call on, also while the sweep is still in flight.
    pub fn sweep_to(&mut self, cutoff_hz: f32, q: f32, frames: u32) -> Result<(), GpuError> {
        if let Some(node) = self.b.node {
            let _g = self.b.cx.control();
            let rc = unsafe { ffi::fwgpu_biquad_sweep(self.b.cx.as_ptr(), node, cutoff_hz, q, frames, 0) };
            self.b.cx.check(rc as i64)?;
        }
        self.cutoff_hz = cutoff_hz;
        self.q = q;
        Ok(())
    }
}
param_node!(GpuDelayNode, "delay", ffi::FWGPU_DELAY, io(1, 64, 1, 64, false),
            "integer-sample delay line with feedback and dry/wet mix; the delay time is fixed at construction",
            [delay_secs, feedback, mix], {set_feedback => (1, feedback), set_mix => (2, mix)});
param_node!(GpuSpatialNode, "spatial", ffi::FWGPU_SPATIAL, io(1, 2, 2, 2, false),
            "3D spatialiser: inverse-distance gain, equal-power pan from the direction cosine, per-ear delay (listener at the origin, -z forward)",
            [x, y, z], {set_x => (0, x), set_y => (1, y), set_z => (2, z)});
impl GpuSpatialNode {
    /// the longest move one message takes, in frames
    pub const MOVE_FRAMES_MAX: u32 = ffi::FWGPU_SPATIAL_MOVE_FRAMES_MAX;
    /// From the next block on, move the source to (`x`, `y`, `z`) over `frames` frames (0: a step, as the setters): the ear gains
    /// travel linearly and per frame, the per-ear delays glide as fractions of a frame — one message for a source that crosses the
    /// stereo image without a click.  A second move starts from where the first stands; a setter during a move ends it.  Before
    /// activation only the target is kept: the node then starts there.  The node's recorded position is the TARGET from this call on.
    pub fn move_to(&mut self, x: f32, y: f32, z: f32, frames: u32) -> Result<(), GpuError> {
        if let Some(node) = self.b.node {
            let _g = self.b.cx.control();
            let rc = unsafe { ffi::fwgpu_spatial_move(self.b.cx.as_ptr(), node, x, y, z, frames, 0) };
            self.b.cx.check(rc as i64)?;
        }
        self.x = x;
        self.y = y;
        self.z = z;
        Ok(())
    }
}

/// FIR / convolution reverb: the impulse response is a [`GpuSample`] named at construction (kept alive by the node).
pub struct GpuFirReverbNode {
    b: Binding,
    ir: GpuSample,
    /// Some: a morph-capable node (two impulse-response slots over one history, include/fwgpu.h "FIR morph")
    morph: Option<FirMorph>,
}
struct FirMorph {
    ir_b: Option<GpuSample>,
    max_taps: u32,
    position: f32,
    law: CrossfadeLaw,
}
impl GpuFirReverbNode {
    pub fn new(cx: &Arc<GpuContext>, impulse_response: GpuSample) -> Self {
        Self { b: Binding::new(cx), ir: impulse_response, morph: None }
    }
    /// Slot A = `ir_a`, slot B = `ir_b` (None: empty), both zero-padded to `max_taps` (0: the longer of the two), blended at
    /// `position` (0 = all A, 1 = all B) under `law`.  A bad value fails activation.
    pub fn new_morph(cx: &Arc<GpuContext>, ir_a: GpuSample, ir_b: Option<GpuSample>, max_taps: u32, position: f32, law: CrossfadeLaw) -> Self {
        Self { b: Binding::new(cx), ir: ir_a, morph: Some(FirMorph { ir_b, max_taps, position, law }) }
    }
    /// From the next block on, move to `position` over `frames` frames (0: a jump) along `curve` (fwgpu_fir_morph); a retarget in
    /// mid-fade starts where the old fade stands.  Before activation only the target is kept: the node then starts at rest there.
    pub fn morph_to(&mut self, position: f32, frames: u32, curve: CrossfadeCurve) -> Result<(), GpuError> {
        let (shape, x1, y1, x2, y2) = match curve {
            CrossfadeCurve::Linear => (0, 0.0, 0.0, 1.0, 1.0),
            CrossfadeCurve::Bezier(x1, y1, x2, y2) => (1, x1, y1, x2, y2),
        };
        if let Some(node) = self.b.node {
            let _g = self.b.cx.control();
            let rc = unsafe { ffi::fwgpu_fir_morph(self.b.cx.as_ptr(), node, position, frames, shape, x1, y1, x2, y2, 0) };
            self.b.cx.check(rc as i64)?;
        }
        if let Some(m) = self.morph.as_mut() {
            m.position = position;
        }
        Ok(())
    }
    /// Exchange the impulse response of a slot nobody hears (0 = A, 1 = B; None: an empty slot B) — fwgpu_fir_set_ir; it takes effect
    /// with the next update.  Before activation the constructor's value is replaced.
    pub fn set_ir(&mut self, slot: u32, sample: Option<GpuSample>) -> Result<(), GpuError> {
        if let Some(node) = self.b.node {
            let _g = self.b.cx.control();
            let id = sample.as_ref().map_or(-1, |s| s.id() as std::os::raw::c_int);
            let rc = unsafe { ffi::fwgpu_fir_set_ir(self.b.cx.as_ptr(), node, slot as std::os::raw::c_int, id) };
            self.b.cx.check(rc as i64)?;
        }
        match (slot, sample, self.morph.as_mut()) {
            (0, Some(s), _) => self.ir = s,
            (1, s, Some(m)) => m.ir_b = s,
            _ => {}
        }
        Ok(())
    }
}
impl AudioNode for GpuFirReverbNode {
    fn debug_name(&self) -> &'static str {
        "fir_reverb"
    }
    fn info(&self) -> AudioNodeInfo {
        io(1, 64, 1, 64, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        // FIR banks run at graph level (one MFMA GEMM per schedule level): use this node under GpuProcessor (B2);
        // fwgpu_node_process refuses it
        match &self.morph {
            None => self.b.activate(ffi::FWGPU_FIR, num_inputs, num_outputs, &[self.ir.id() as f32]),
            Some(m) => {
                let ir_b = m.ir_b.as_ref().map_or(-1.0, |s| s.id() as f32);
                self.b.activate(ffi::FWGPU_FIR, num_inputs, num_outputs, &[self.ir.id() as f32, ir_b, m.max_taps as f32, m.position, m.law as i32 as f32])
            }
        }
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

/// Polyphase resampling source (varispeed / rate conversion of a sample): 32.32 fixed-point position, 32 x 16 Kaiser bank.
pub struct GpuResamplerNode {
    b: Binding,
    source: GpuSample,
    ratio: f32,
    looping: bool,
    playing: bool,
}
impl GpuResamplerNode {
    pub fn new(cx: &Arc<GpuContext>, source: GpuSample, ratio: f32, looping: bool, playing: bool) -> Self {
        Self { b: Binding::new(cx), source, ratio, looping, playing }
    }
    pub fn set_ratio(&mut self, ratio: f32) {
        self.ratio = ratio;
        let _ = self.b.set_param(1, ratio);
    }
    pub fn set_playing(&mut self, playing: bool) {
        self.playing = playing;
        let _ = self.b.set_param(3, playing as i32 as f32);
    }
    pub fn seek(&mut self, source_frame: f32) {
        let _ = self.b.set_param(4, source_frame);
    }
    /// the longest glide one message takes, in frames
    pub const GLIDE_FRAMES_MAX: u32 = ffi::FWGPU_RESAMPLER_GLIDE_FRAMES_MAX;
    /// From the next block on, move the ratio to `ratio` over `frames` output frames, linearly in the 32.32 step (0: a step, as
    /// `set_ratio`) — one message for a pitch that moves every frame (Doppler).  A second glide starts from the step the first has
    /// reached.  Before activation only the target is kept: the node then starts at that ratio.  The node's recorded ratio is the
    /// TARGET from this call on, also while the glide is still in flight.
    pub fn glide_to(&mut self, ratio: f32, frames: u32) -> Result<(), GpuError> {
        if let Some(node) = self.b.node {
            let _g = self.b.cx.control();
            let rc = unsafe { ffi::fwgpu_resampler_glide(self.b.cx.as_ptr(), node, ratio, frames, 0) };
            self.b.cx.check(rc as i64)?;
        }
        self.ratio = ratio;
        Ok(())
    }
}
impl AudioNode for GpuResamplerNode {
    fn debug_name(&self) -> &'static str {
        "resampler"
    }
    fn info(&self) -> AudioNodeInfo {
        io(0, 0, 1, 64, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(
            ffi::FWGPU_RESAMPLER,
            num_inputs,
            num_outputs,
            &[self.source.id() as f32, self.ratio, self.looping as i32 as f32, self.playing as i32 as f32],
        )
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

/// Level meter (SPEC, DESIGN.md §6 of the fwgpu repository): per block and input channel the peak, the f32 sum of squares and the
/// number of samples over 1.0, measured on the device.  `num_outputs == num_inputs` passes the audio through, `num_outputs == 0` is a
/// tap.  Readings are recorded by the whole-graph executor ([`crate::GpuProcessor`], B2); a block run through `fwgpu_node_process`
/// (B1) passes through unrecorded.
pub struct GpuMeterNode {
    b: Binding,
    ring_blocks: u32,
    spectrum: Option<(u32, u32)>,
    num_inputs: usize,
}
/// one record per (block, input channel)
pub type MeterReading = ffi::fwgpu_meter_reading;
impl GpuMeterNode {
    /// `ring_blocks` (1..=65536): how many blocks of readings the node retains
    pub fn new(cx: &Arc<GpuContext>, ring_blocks: u32) -> Self {
        Self { b: Binding::new(cx), ring_blocks, spectrum: None, num_inputs: 0 }
    }
    /// A spectrum meter as well (at most [`ffi::FWGPU_SPECTRUM_CH_MAX`] channels): per block and input channel the band powers of a
    /// Hann-windowed FFT over the channel's last `fft_size` frames (256, 512, 1024, 2048 or 4096), `bands` log-spaced bands over bins
    /// `1..=fft_size/2` (0: every bin, DC included).  A full-scale sine on a bin centre reads 1.0.
    pub fn with_spectrum(cx: &Arc<GpuContext>, ring_blocks: u32, fft_size: u32, bands: u32) -> Self {
        Self { b: Binding::new(cx), ring_blocks, spectrum: Some((fft_size, bands)), num_inputs: 0 }
    }
    /// The floats of one spectrum record and the band edges `e[0..=B]`: band `b` covers bins `e[b] .. e[b+1] - 1`, bin `k` is centred on
    /// `k * sample_rate / fft_size` Hz.  Audio-side call.
    pub fn spectrum_layout(&self) -> Result<(usize, Vec<u32>), GpuError> {
        let node = self.b.node.unwrap_or(-1);
        let cx = self.b.cx.as_ptr();
        let bands = self.b.cx.check(unsafe { ffi::fwgpu_spectrum_layout(cx, node, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), 0) } as i64)? as usize;
        let mut edges = vec![0u32; bands + 1];
        self.b.cx.check(unsafe { ffi::fwgpu_spectrum_layout(cx, node, std::ptr::null_mut(), std::ptr::null_mut(), edges.as_mut_ptr(), edges.len() as u32) } as i64)?;
        Ok((bands, edges))
    }
    /// The spectrum records of blocks `[first_block, first_block + n)`, `out[(i * num_inputs + c) * B + b]`, for the `n <= num_blocks`
    /// of them that exist yet, `B` (the floats of one record) and the context's block count.  Audio-side call, as [`GpuMeterNode::read`].
    pub fn spectrum(&self, first_block: u64, num_blocks: u32) -> Result<(Vec<f32>, usize, u64), GpuError> {
        let node = self.b.node.unwrap_or(-1);
        let (bands, _) = self.spectrum_layout()?;
        let mut out = vec![0f32; num_blocks as usize * self.num_inputs.max(1) * bands];
        let mut done: u64 = 0;
        let n = self.b.cx.check(unsafe { ffi::fwgpu_spectrum_read(self.b.cx.as_ptr(), node, first_block, num_blocks, out.as_mut_ptr(), &mut done) })?;
        out.truncate(n as usize * self.num_inputs * bands);
        Ok((out, bands, done))
    }
    /// The records of blocks `[first_block, first_block + n)`, `out[i * num_inputs + c]`, for the `n <= num_blocks` of them that exist
    /// yet, and the context's block count.  Audio-side call: waits for the context's stream.
    pub fn read(&self, first_block: u64, num_blocks: u32) -> Result<(Vec<MeterReading>, u64), GpuError> {
        let node = self.b.node.unwrap_or(-1);
        let mut out = vec![MeterReading::default(); num_blocks as usize * self.num_inputs.max(1)];
        let mut done: u64 = 0;
        let n = self.b.cx.check(unsafe { ffi::fwgpu_meter_read(self.b.cx.as_ptr(), node, first_block, num_blocks, out.as_mut_ptr(), &mut done) })?;
        out.truncate(n as usize * self.num_inputs);
        Ok((out, done))
    }
    /// core/util.rs gain_to_db of a reading's peak
    pub fn peak_db(r: &MeterReading) -> f32 {
        firewheel_core::util::gain_to_db(r.peak)
    }
    /// ... and of its rms = sqrt(sum_squares / frames)
    pub fn rms_db(r: &MeterReading) -> f32 {
        firewheel_core::util::gain_to_db((r.sum_squares / r.frames as f32).sqrt())
    }
}
impl AudioNode for GpuMeterNode {
    fn debug_name(&self) -> &'static str {
        "meter"
    }
    fn info(&self) -> AudioNodeInfo {
        io(1, 64, 0, 64, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.num_inputs = num_inputs;
        match self.spectrum {
            None => self.b.activate(ffi::FWGPU_METER, num_inputs, num_outputs, &[self.ring_blocks as f32]),
            Some((n, bands)) => self.b.activate(ffi::FWGPU_METER, num_inputs, num_outputs, &[self.ring_blocks as f32, n as f32, bands as f32]),
        }
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

/// Look-ahead limiter (SPEC, DESIGN.md §6 of the fwgpu repository): linked channels, brickwall at `ceiling` (linear), a hold of
/// `hold_frames`, [`GpuLimiterNode::LATENCY_FRAMES`] frames of latency.  A sliding minimum of the target gain and a 64-term moving average:
/// no recurrence in time, so the blocks of a batch render in parallel on the device.  As many outputs as inputs, 1..=8.
pub struct GpuLimiterNode {
    b: Binding,
    ceiling: f32,
    hold_frames: u32,
}
impl GpuLimiterNode {
    /// what the output is late by
    pub const LATENCY_FRAMES: u32 = ffi::FWGPU_LIMITER_LATENCY;
    /// `ceiling`: linear, finite, 0.001..=1000; `hold_frames`: 0..=1920.  Anything else fails activation.
    pub fn new(cx: &Arc<GpuContext>, ceiling: f32, hold_frames: u32) -> Self {
        Self { b: Binding::new(cx), ceiling, hold_frames }
    }
    /// the ceiling in decibels, through core/util.rs db_to_gain (what [`GpuMeterNode::peak_db`] inverts)
    pub fn with_ceiling_db(cx: &Arc<GpuContext>, ceiling_db: f32, hold_frames: u32) -> Self {
        Self::new(cx, firewheel_core::util::db_to_gain(ceiling_db), hold_frames)
    }
}
impl AudioNode for GpuLimiterNode {
    fn debug_name(&self) -> &'static str {
        "limiter"
    }
    fn info(&self) -> AudioNodeInfo {
        io(1, 8, 1, 8, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(ffi::FWGPU_LIMITER, num_inputs, num_outputs, &[self.ceiling, self.hold_frames as f32])
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

/// Sidechain ducker (SPEC, DESIGN.md §6 of the fwgpu repository): while the key bus is above `threshold` the main bus is turned down
/// to `depth` (linear gain while ducked) — down over `attack_frames`, held for `hold_frames`, back over `release_frames`.  The gain is
/// a function of integer counts over windows of the key's gate bits: no recurrence in time, so the blocks of a batch render in
/// parallel on the device; no latency.  Inputs `0..n` are the main bus, inputs `n..n + k` the key (never heard); `n` outputs;
/// `n` and `k` in 1..=8.
pub struct GpuDuckerNode {
    b: Binding,
    threshold: f32,
    depth: f32,
    attack_frames: u32,
    release_frames: u32,
    hold_frames: u32,
}
impl GpuDuckerNode {
    /// `threshold`: linear, finite, 1e-6..=1000; `depth`: 0..=1; `attack_frames`, `release_frames`: 1..=32768; `hold_frames`:
    /// 0..=32768.  Anything else fails activation.
    pub fn new(cx: &Arc<GpuContext>, threshold: f32, depth: f32, attack_frames: u32, release_frames: u32, hold_frames: u32) -> Self {
        Self { b: Binding::new(cx), threshold, depth, attack_frames, release_frames, hold_frames }
    }
    /// threshold and depth in decibels, through core/util.rs db_to_gain
    pub fn with_db(cx: &Arc<GpuContext>, threshold_db: f32, depth_db: f32, attack_frames: u32, release_frames: u32, hold_frames: u32) -> Self {
        Self::new(cx, firewheel_core::util::db_to_gain(threshold_db), firewheel_core::util::db_to_gain(depth_db), attack_frames,
                  release_frames, hold_frames)
    }
    /// a time in seconds as whole frames of `sample_rate` (what the three `_frames` arguments take)
    pub fn secs_to_frames(secs: f64, sample_rate: u32) -> u32 {
        (secs * sample_rate as f64).round().max(0.0) as u32
    }
}
impl AudioNode for GpuDuckerNode {
    fn debug_name(&self) -> &'static str {
        "ducker"
    }
    fn info(&self) -> AudioNodeInfo {
        io(2, 16, 1, 8, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(
            ffi::FWGPU_DUCKER,
            num_inputs,
            num_outputs,
            &[self.threshold, self.depth, self.attack_frames as f32, self.release_frames as f32, self.hold_frames as f32],
        )
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

/// Bus compressor (SPEC, DESIGN.md §6 of the fwgpu repository): self-keyed with linked channels.  Above `threshold` the level rises
/// `ratio` times slower, through a soft knee `knee_db` wide; the gain comes down over `attack_frames`, stays for `hold_frames` and comes
/// back over `release_frames`; `makeup` scales the result.  The curve is a table built on the host, the gain a function of integer sums
/// over windows of the quantised target: no recurrence in time, so the blocks of a batch render in parallel on the device; no
/// latency.  As many outputs as inputs, 1..=8.
pub struct GpuCompressorNode {
    b: Binding,
    threshold: f32,
    ratio: f32,
    knee_db: f32,
    attack_frames: u32,
    release_frames: u32,
    hold_frames: u32,
    makeup: f32,
}
impl GpuCompressorNode {
    /// the longest attack / release window and the longest hold, in frames
    pub const WIN_MAX: u32 = ffi::FWGPU_COMPRESSOR_WIN_MAX;
    pub const HOLD_MAX: u32 = ffi::FWGPU_COMPRESSOR_HOLD_MAX;
    /// `threshold`: linear, finite, 1e-6..=1000; `ratio`: 1..=1000; `knee_db`: 0..=24; `attack_frames`, `release_frames`:
    /// 1..=[`GpuCompressorNode::WIN_MAX`]; `hold_frames`: 0..=[`GpuCompressorNode::HOLD_MAX`]; `makeup`: linear, 0.001..=1000.
    /// Anything else fails activation.
    #[allow(clippy::too_many_arguments)]
    pub fn new(cx: &Arc<GpuContext>, threshold: f32, ratio: f32, knee_db: f32, attack_frames: u32, release_frames: u32, hold_frames: u32,
               makeup: f32) -> Self {
        Self { b: Binding::new(cx), threshold, ratio, knee_db, attack_frames, release_frames, hold_frames, makeup }
    }
    /// threshold and makeup in decibels, through core/util.rs db_to_gain
    #[allow(clippy::too_many_arguments)]
    pub fn with_db(cx: &Arc<GpuContext>, threshold_db: f32, ratio: f32, knee_db: f32, attack_frames: u32, release_frames: u32, hold_frames: u32,
                   makeup_db: f32) -> Self {
        Self::new(cx, firewheel_core::util::db_to_gain(threshold_db), ratio, knee_db, attack_frames, release_frames, hold_frames,
                  firewheel_core::util::db_to_gain(makeup_db))
    }
    /// a time in seconds as whole frames of `sample_rate` (what the three `_frames` arguments take)
    pub fn secs_to_frames(secs: f64, sample_rate: u32) -> u32 {
        (secs * sample_rate as f64).round().max(0.0) as u32
    }
}
impl AudioNode for GpuCompressorNode {
    fn debug_name(&self) -> &'static str {
        "compressor"
    }
    fn info(&self) -> AudioNodeInfo {
        io(1, 8, 1, 8, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(
            ffi::FWGPU_COMPRESSOR,
            num_inputs,
            num_outputs,
            &[self.threshold, self.ratio, self.knee_db, self.attack_frames as f32, self.release_frames as f32, self.hold_frames as f32, self.makeup],
        )
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

/// Latency compensation (SPEC, DESIGN.md §6 of the fwgpu repository): a pure delay of `frames` whole frames, a copy with no arithmetic —
/// what a bus needs that is summed with a bus a [`GpuLimiterNode`] has made [`GpuLimiterNode::LATENCY_FRAMES`] frames late.  No
/// recurrence in time, so every block of a batch renders in parallel on the device.  An output block is flagged silent exactly when
/// the `frames` frames in front of it and the block itself were.  As many outputs as inputs, 1..=8.
pub struct GpuDelayCompNode {
    b: Binding,
    frames: u32,
}
impl GpuDelayCompNode {
    /// the largest delay one node takes
    pub const MAX_FRAMES: u32 = ffi::FWGPU_DELAY_COMP_MAX;
    /// `frames`: 0..=[`GpuDelayCompNode::MAX_FRAMES`] (0 is the identity).  Anything else fails activation.
    pub fn new(cx: &Arc<GpuContext>, frames: u32) -> Self {
        Self { b: Binding::new(cx), frames }
    }
    /// the delay that aligns a bus with one a limiter has made late
    pub fn for_limiter(cx: &Arc<GpuContext>) -> Self {
        Self::new(cx, GpuLimiterNode::LATENCY_FRAMES)
    }
    /// what the output is late by
    pub fn latency_frames(&self) -> u32 {
        self.frames
    }
}
impl AudioNode for GpuDelayCompNode {
    fn debug_name(&self) -> &'static str {
        "delay_comp"
    }
    fn info(&self) -> AudioNodeInfo {
        io(1, 8, 1, 8, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(ffi::FWGPU_DELAY_COMP, num_inputs, num_outputs, &[self.frames as f32])
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}

/// Crossfader (SPEC, DESIGN.md §6 of the fwgpu repository): two buses blended along an automated curve.  Inputs `0..n` are bus A,
/// inputs `n..2n` bus B; `n` outputs, `n` in 1..=8.  Position 0 is all A, 1 all B.  The position is a pure function of the node's
/// frame count, so a fade in flight renders block-parallel on the device; at rest at an end the output is a copy of one bus.  With
/// bus B left unconnected the node is a fader of bus A with the same curves.
pub struct GpuCrossfadeNode {
    b: Binding,
    position: f32,
    law: CrossfadeLaw,
}
/// how the position becomes the two gains: `Linear` a = 1 - p, b = p; `EqualPower` a = sqrt(1 - p), b = sqrt(p)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum CrossfadeLaw {
    Linear = 0,
    EqualPower = 1,
}
/// the shape of a segment: a straight line, or a cubic Bézier easing from (0, 0) to (1, 1) through (x1, y1) and (x2, y2)
/// (x in 0..=1, y in -1..=2; the position itself is clamped to 0..=1)
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum CrossfadeCurve {
    Linear,
    Bezier(f32, f32, f32, f32),
}
impl CrossfadeCurve {
    pub const EASE_IN: Self = Self::Bezier(0.42, 0.0, 1.0, 1.0);
    pub const EASE_OUT: Self = Self::Bezier(0.0, 0.0, 0.58, 1.0);
    pub const EASE_IN_OUT: Self = Self::Bezier(0.42, 0.0, 0.58, 1.0);
}
impl GpuCrossfadeNode {
    /// the longest segment one message takes, in frames
    pub const FRAMES_MAX: u32 = ffi::FWGPU_CROSSFADE_FRAMES_MAX;
    /// `position`: 0..=1.  Anything else fails activation.
    pub fn new(cx: &Arc<GpuContext>, position: f32, law: CrossfadeLaw) -> Self {
        Self { b: Binding::new(cx), position, law }
    }
    /// the target of the last message (or the constructor's position)
    pub fn position(&self) -> f32 {
        self.position
    }
    /// From the next block on, move to `position` over `frames` frames (0: a jump) along `curve`; a retarget in mid-fade starts where
    /// the old fade stands.  Before activation only the target is kept: the node then starts at rest there.
    pub fn crossfade_to(&mut self, position: f32, frames: u32, curve: CrossfadeCurve) -> Result<(), GpuError> {
        let (shape, x1, y1, x2, y2) = match curve {
            CrossfadeCurve::Linear => (0, 0.0, 0.0, 1.0, 1.0),
            CrossfadeCurve::Bezier(x1, y1, x2, y2) => (1, x1, y1, x2, y2),
        };
        if let Some(node) = self.b.node {
            let _g = self.b.cx.control();
            let rc = unsafe { ffi::fwgpu_crossfade_to(self.b.cx.as_ptr(), node, position, frames, shape, x1, y1, x2, y2, 0) };
            self.b.cx.check(rc as i64)?;
        }
        self.position = position;
        Ok(())
    }
    /// ... over `secs` seconds, rounded to whole frames of `sample_rate`
    pub fn crossfade_to_secs(&mut self, position: f32, secs: f64, sample_rate: u32, curve: CrossfadeCurve) -> Result<(), GpuError> {
        self.crossfade_to(position, (secs * sample_rate as f64).round().max(0.0) as u32, curve)
    }
}
impl AudioNode for GpuCrossfadeNode {
    fn debug_name(&self) -> &'static str {
        "crossfade"
    }
    fn info(&self) -> AudioNodeInfo {
        io(2, 16, 1, 8, false)
    }
    fn activate(&mut self, _sr: u32, _mbf: usize, num_inputs: usize, num_outputs: usize) -> Result<Box<dyn AudioNodeProcessor>, Box<dyn Error>> {
        self.b.activate(ffi::FWGPU_CROSSFADE, num_inputs, num_outputs, &[self.position, self.law as i32 as f32])
    }
    fn deactivate(&mut self, _p: Option<Box<dyn AudioNodeProcessor>>) {
        self.b.deactivate()
    }
}
