"""Samplers (reference: owl_wms/sampling/__init__.py:1-39).

Implemented on libowlk's KV-cache decode path: ``av_caching`` (AVCachingSamplerV2, the registry
entry the reference resolves it to), ``av_stream`` (stream.py: the same sampler on a ring cache with a
RoPE rebase, for rollouts past ``n_frames``), ``audio_caching``, ``audio_stream`` (stream.py
AudioStreamSampler: the audio sampler on a ring cache, for rollouts past ``n_frames``), and the audio + video core's samplers
``av_window`` / ``av_causal`` / ``av_causal_no_cfg`` (av_window.py; the causal ones decode on the
MMDiT's fused joint-frame path) and ``av_audio_stream`` (stream.py AVStreamSampler: endless audio + video
streaming on a ring cache, each frame cached once, on either backbone of the core).  The one-step variant is outside this build's scope (SURVEY.md
§8(f); the reference's import of it is broken).
"""

# the samplers that take the (video, audio) core: sampler(model, video, audio, mouse, btn)
AV_WINDOW_SAMPLERS = {"av_window": "AVWindowSampler", "av_causal": "CausalAVWindowSampler",
                      "av_causal_no_cfg": "CausalAVWindowSamplerNoCFG"}
# every sampler with that call signature (AVRFTTrainer's eval step takes any of them)
AV_CORE_SAMPLERS = tuple(AV_WINDOW_SAMPLERS) + ("av_audio_stream",)


def get_sampler_cls(sampler_id):
    if sampler_id == "av_caching":
        from .av_caching_v2 import AVCachingSamplerV2
        return AVCachingSamplerV2
    if sampler_id == "av_stream":
        from .stream import StreamSampler
        return StreamSampler
    if sampler_id == "av_audio_stream":
        from .stream import AVStreamSampler
        return AVStreamSampler
    if sampler_id == "audio_caching":
        from .audio_caching import AudioCachingSampler
        return AudioCachingSampler
    if sampler_id == "audio_stream":
        from .stream import AudioStreamSampler
        return AudioStreamSampler
    if sampler_id in AV_WINDOW_SAMPLERS:
        from . import av_window
        return getattr(av_window, AV_WINDOW_SAMPLERS[sampler_id])
    if sampler_id == "av_caching_one_step":
        raise NotImplementedError(f"sampler {sampler_id!r} is out of scope for the MI355X build (SURVEY.md §8(f))")
    raise ValueError(f"unknown sampler_id {sampler_id!r}")
