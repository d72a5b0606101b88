"""conceptattention_amd: MI355X-native ConceptAttention hot path.

Public surface mirrors the reference package (`concept_attention/__init__.py:2`):
``from conceptattention_amd import ConceptAttentionFluxPipeline``.  Importing the package does not
touch the GPU; the HIP library is loaded on first use and its absence is a hard error.
"""
from .params import (AutoEncoderParams, ClipTextParams, FluxParams, T5Params, ae_params, clip_params, configs,  # noqa: F401
                     t5_params, tiny_clip_params, tiny_params, tiny_t5_params)


def __getattr__(name):  # lazy: keep `import conceptattention_amd` light for host-only tools
    if name in ("ConceptAttentionFluxPipeline", "ConceptAttentionPipelineOutput", "ImageTrace"):
        from . import pipeline
        return getattr(pipeline, name)
    if name in ("HipFluxDiT", "FluxWeights", "HeatmapRequest", "StepTrace"):
        from . import flux_dit
        return getattr(flux_dit, name)
    if name in ("FluxGenerator", "load_flow_model"):
        from . import image_generator
        return getattr(image_generator, name)
    if name in ("AutoEncoder", "load_ae", "synthetic_ae_state_dict", "ae_state_dict_spec"):
        from . import vae
        return getattr(vae, name)
    if name in ("T5Encoder", "HipTextEncoder", "ToyByteTokenizer", "load_t5", "synthetic_t5_state_dict", "t5_state_dict_spec"):
        from . import t5
        return getattr(t5, name)
    if name in ("ClipTextEncoder", "HipClipEmbedder", "ToyClipTokenizer", "load_clip", "synthetic_clip_state_dict",
                "clip_state_dict_spec"):
        from . import clip
        return getattr(clip, name)
    if name in ("ConceptAttentionSegmentationModel", "MultiClassScores", "DeviceMultiClassScores",
                "map_predictions_to_class_indices", "multiclass_table"):
        from . import segmentation
        return getattr(segmentation, name)
    if name in ("RawOutputSpaceSegmentationModel", "RawValueSpaceSegmentationModel", "RawCrossAttentionSegmentationModel",
                "DAAMFluxSegmentationModel"):
        from . import baselines
        return getattr(baselines, name)
    if name == "concept_attention_frames":
        from .video import concept_attention_frames
        return concept_attention_frames
    if name == "compute_heatmaps_from_vectors":
        from .heatmaps import compute_heatmaps_from_vectors
        return compute_heatmaps_from_vectors
    raise AttributeError(name)
