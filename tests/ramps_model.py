"""The five per-frame ramps in ONE reference engine (CMD_SMP_FADE, CMD_RS_GLIDE, CMD_BQ_SWEEP, CMD_SP_MOVE,
CMD_SMP_STREAM).  Nothing is restated here: the node classes stay in the five model files and `RampsRefEngine.add_node` picks among
them by kind; the message methods, SweepRefEngine._block's `process_batch` substitution and `process_blocks_flags` are the single
engines' own, inherited.  `Tagged` and `GpuRamps` are the five `Tagged` / `Gpu*` wrappers in one, the same way.
tests/test_ramps_together.py pins this engine against each single engine before it compares anything with it."""
import fwapi
import bq_sweep_model as bqm
import rs_glide_model as rgm
import sampler_fade_model as sfm
import sp_move_model as spm
import stream_source_model as ssm

NODE_CLASSES = {fwapi.SAMPLER: ssm.StreamSamplerNode,      # (it extends the fade model's node: the envelope is there too)
                fwapi.BIQUAD: bqm.SweepBiquadNode,
                fwapi.RESAMPLER: rgm.GlideResamplerNode,
                fwapi.SPATIAL: spm.MoveSpatialNode}


class RampsRefEngine(ssm.StreamRefEngine, bqm.SweepRefEngine, rgm.GlideRefEngine, spm.MoveRefEngine):
    """fade / new_stream / sampler_set_stream (StreamRefEngine over FadeRefEngine), sweep / _block / node_process (SweepRefEngine),
    glide (GlideRefEngine), move (MoveRefEngine), process_blocks_flags (the same text in each)"""

    def add_node(self, kind, n_in, n_out, params=()):
        if kind in NODE_CLASSES:
            return self._add(NODE_CLASSES[kind](self, n_in, n_out, [float(p) for p in params]))
        return bqm.refmodel.RefEngine.add_node(self, kind, n_in, n_out, params)


class Tagged(sfm.Tagged, bqm.Tagged, rgm.Tagged, spm.Tagged):
    """messages tagged with a block of the next call (deferral by at_block, as each model's own): fade, sweep, glide, move; the stream
    calls go straight to the engine (a write is seen at the top of the next block)"""


class GpuRamps(sfm.GpuFade, bqm.GpuSweep, rgm.GpuGlide, spm.GpuMove):
    """a GpuEngine (or the host-only harness engine) with fade, sweep, glide and move under the models' names; streams are the
    context's own (`cx.new_stream`, sampler_set_sample with the stream's id), as tests/test_stream_source.py's Feed uses them"""
