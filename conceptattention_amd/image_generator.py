"""FluxGenerator: host-side mirror of the reference's generator object
(``concept_attention/image_generator.py:64-205``) for the HIP path.

Same constructor arguments (``model_name, device, offload, attention_block_class, dit_class``) and the
same ``generate_image(width, height, num_steps, guidance, seed, prompt, concepts, ...)`` ->
``(image, concept_attention_dict)`` contract, where the dict holds the four vector stacks
``[steps, 19, 1, ...]`` that ``compute_heatmaps_from_vectors`` consumes.  What is NOT re-stated: the
HuggingFace downloads (`load_t5/load_clip/load_ae/hf_hub_download`, `:19-62`; unavailable offline) -- the
text encoder and autoencoder are injectable (``autoencoder`` also takes "synthetic" or a ``.safetensors`` path and
then builds the HIP ``vae.AutoEncoder``; ``text_encoder`` takes a ``t5.HipTextEncoder``, whose T5 side is the HIP
encoder of ``t5.py`` on local weights and whose CLIP side may be the HIP encoder of ``clip.py``, or "synthetic-t5", the
T5 encoder on synthetic weights behind a toy tokenizer, or "synthetic-t5-clip", that plus a synthetic CLIP text encoder
for the pooled ``vec``).  By default the text encoder is still the seeded-noise stand-in and the unpacked latent is
returned instead of an image.  Also not re-stated: the
`model.cpu()` / `.to(device)` round trip of the 23.8 GB weights on every call (`:183,194`), which a
288 GB device does not need.
"""
from __future__ import annotations

import os
import time
from collections import OrderedDict

import torch

from . import sampling
from .flux_dit import HipFluxDiT, on_own_device
from .params import T5_TOKENS, ae_params, configs


def load_flow_model(name: str, device="cuda", hf_download: bool = True, attention_block_class=None,
                    dit_class=HipFluxDiT, weights="synthetic", weight_seed: int = 0, params=None,
                    residual_dtype=torch.float32):
    """Counterpart of load_flow_model (image_generator.py:19-47): builds ``dit_class(params)`` and fills
    it from ``weights``: "synthetic", a flux1-*.safetensors path (env FLUX_SCHNELL / FLUX_DEV are honoured
    like flux/util.py:33,65), or a state dict.  Nothing is downloaded."""
    import os
    p = params if params is not None else configs[name]
    model = (dit_class(p, device, residual_dtype=residual_dtype) if dit_class is HipFluxDiT
             else dit_class(p, attention_block_class=attention_block_class))
    env = {"flux-schnell": "FLUX_SCHNELL", "flux-dev": "FLUX_DEV"}.get(name)
    if isinstance(weights, str) and weights == "synthetic" and env and os.getenv(env):
        weights = os.getenv(env)
    if isinstance(weights, str) and weights == "synthetic":
        model.weights.init_synthetic(weight_seed)
    elif isinstance(weights, str):
        from safetensors.torch import load_file
        model.load_state_dict(load_file(weights, device=str(device)), strict=False)
    elif weights is not None:
        model.load_state_dict(weights, strict=False)
    return model


class ConceptCache:
    """Bounded LRU of concept first-token vectors (bf16 [context_dim] on the device, 8 KB each at 4096), keyed by the
    concept string.  It belongs to one encoder object: ``bind`` drops every entry when another one shows up."""

    def __init__(self, max_entries: int = 4096):
        if max_entries < 1:
            raise ValueError("ConceptCache: max_entries must be >= 1")
        self.max_entries = int(max_entries)
        self._entries: OrderedDict = OrderedDict()
        self._owner = None

    def bind(self, encoder) -> None:
        if encoder is not self._owner:
            self._entries.clear()
            self._owner = encoder

    def get(self, text: str):
        v = self._entries.get(text)
        if v is not None:
            self._entries.move_to_end(text)
        return v

    def put(self, text: str, vector) -> None:
        self._entries[text] = vector
        self._entries.move_to_end(text)
        while len(self._entries) > self.max_entries:
            self._entries.popitem(last=False)

    def __len__(self):
        return len(self._entries)

    def __contains__(self, text):
        return text in self._entries


class FluxGenerator:
    def __init__(self, model_name: str, device, offload: bool = False, attention_block_class=None,
                 dit_class=HipFluxDiT, weights="synthetic", weight_seed: int = 0, text_encoder=None,
                 autoencoder=None, params=None, n_text_tokens=None, residual_dtype=torch.float32,
                 t5_precision: str = "bf16"):
        """``t5_precision``: the precision of the T5 encoder built for ``text_encoder="synthetic-t5"`` /
        ``"synthetic-t5-clip"`` ("bf16", or "fp8": t5.T5Encoder's opt-in e4m3 projections); an encoder object passed in
        carries its own precision and must be left at the default here."""
        from .pipeline import SyntheticTextEncoder
        if t5_precision != "bf16" and not isinstance(text_encoder, str):
            raise ValueError("t5_precision applies to the T5 encoder built from a text_encoder name; an encoder object "
                             "(or the seeded-noise stand-in) has none to set")
        self.device = torch.device(device)
        self.offload = offload
        self.model_name = model_name
        self.is_schnell = model_name == "flux-schnell"
        self.params = params if params is not None else configs[model_name]
        self.model = load_flow_model(model_name, self.device, attention_block_class=attention_block_class,
                                     dit_class=dit_class, weights=weights, weight_seed=weight_seed,
                                     params=self.params, residual_dtype=residual_dtype)
        n_tok = n_text_tokens or T5_TOKENS.get(model_name, 256)
        if isinstance(text_encoder, str):
            if text_encoder not in ("synthetic-t5", "synthetic-t5-clip"):
                raise ValueError(f"text_encoder: unknown name {text_encoder!r} (\"synthetic-t5\", \"synthetic-t5-clip\", "
                                 "or an encoder object)")
            from .t5 import synthetic_text_encoder
            clip = None
            if text_encoder == "synthetic-t5-clip":
                from .clip import synthetic_clip_embedder
                clip = synthetic_clip_embedder(self.params.vec_in_dim, self.device, weight_seed)
            text_encoder = synthetic_text_encoder(self.params.context_in_dim, n_tok, self.device,
                                                  self.params.vec_in_dim, weight_seed, clip=clip,
                                                  t5_precision=t5_precision)
        enc = text_encoder or SyntheticTextEncoder(n_tok, self.params.context_in_dim, self.params.vec_in_dim,
                                                   self.device)
        self.text_encoder = enc
        self.t5, self.clip = enc.t5, enc.clip
        if isinstance(autoencoder, (str, os.PathLike)):   # "synthetic" or a .safetensors path: the HIP autoencoder
            from .vae import load_ae
            autoencoder = load_ae(model_name if model_name in ae_params else "flux-schnell", self.device,
                                  weights=str(autoencoder), seed=weight_seed)
        self.ae = autoencoder
        self.nsfw_classifier = None
        self.concept_cache = ConceptCache()
        self.t5_sequences_encoded = 0     # sequences embed_many actually sent through the T5 encoder (for tests)

    def embed(self, prompt: str, concepts):
        """prepare()'s text side + embed_concepts (flux/sampling.py:47-55, concept_attention/utils.py:6-33).  A text
        encoder with ``t5_many`` encodes the prompt and every concept in ONE forward; any other one is called once per
        string, as the reference does."""
        many = getattr(self.text_encoder, "t5_many", None)
        if many is not None:
            both, vec = many([prompt, *concepts]), self.clip(prompt)
            txt, con = both[:1], both[1:, 0, :].unsqueeze(0)
        else:
            txt, vec = self.t5(prompt), self.clip(prompt)
            con = torch.stack([self.t5(c)[0, 0, :] for c in concepts]).unsqueeze(0)
        con, con_ids, con_vec = sampling.concept_inputs(con, vec)
        return txt, vec, con, con_ids, con_vec

    def embed_many(self, prompts, concepts_per_item):
        """``embed`` for several items: [(txt, vec, con, con_ids, con_vec), ...], each entry bit for bit what
        ``embed(prompt, concepts)`` returns for that item.  ONE T5 call over the distinct strings that are needed --
        every distinct prompt, and the concepts ``concept_cache`` does not hold yet -- and one ``clip_many`` call over
        the distinct prompts.  (The T5 encoder gives a sequence the same bits whatever else is in the call.)  A text
        encoder without ``t5_many`` is called through ``embed`` per item."""
        prompts, concepts_per_item = list(prompts), [list(c) for c in concepts_per_item]
        if len(prompts) != len(concepts_per_item):
            raise ValueError("embed_many: one concept list per prompt")
        many = getattr(self.text_encoder, "t5_many", None)
        if many is None:
            return [self.embed(p, c) for p, c in zip(prompts, concepts_per_item)]
        uniq_prompts = list(dict.fromkeys(prompts))
        both, con_vecs = self._t5_with_concepts(uniq_prompts, concepts_per_item)
        txts = {p: both[i:i + 1] for i, p in enumerate(uniq_prompts)}
        clip_many = getattr(getattr(self.text_encoder, "clip_embedder", None), "clip_many", None)
        if clip_many is not None:
            pooled = clip_many(uniq_prompts)
            vecs = {p: pooled[i:i + 1] for i, p in enumerate(uniq_prompts)}
        else:
            vecs = {p: self.clip(p) for p in uniq_prompts}
        out = []
        for p, cs in zip(prompts, concepts_per_item):
            con = torch.stack([con_vecs[c] for c in cs]).unsqueeze(0)
            out.append((txts[p], vecs[p], *sampling.concept_inputs(con, vecs[p])))
        return out

    def _t5_with_concepts(self, sequences, concepts_per_item):
        """ONE ``t5_many`` call over ``sequences`` and the concepts ``concept_cache`` does not hold yet: (the encoder's
        output, whose first rows are the sequences'; concept string -> its first-token vector).  No call when there is
        nothing to encode."""
        cache = self.concept_cache
        cache.bind(self.text_encoder)
        concepts = list(dict.fromkeys(c for cs in concepts_per_item for c in cs))
        # read every cached vector BEFORE anything is inserted: an insertion may evict an entry this call still needs
        con_vecs = {c: cache.get(c) for c in concepts}
        new = [c for c in concepts if con_vecs[c] is None]
        both = self.text_encoder.t5_many(list(sequences) + new) if (sequences or new) else None
        self.t5_sequences_encoded += len(sequences) + len(new)
        for j, c in enumerate(new):
            con_vecs[c] = both[len(sequences) + j, 0, :].clone()     # (a copy: the entry must not pin the whole batch)
            cache.put(c, con_vecs[c])
        return both, con_vecs

    def embed_concepts_many(self, concepts_per_item) -> list:
        """The concept side of ``embed_many`` alone, for a re-query: per item (con (1,C,4096), con_ids (1,C,3)), the
        same bits ``embed`` / ``embed_many`` give those concept strings; the prompt is not encoded."""
        concepts_per_item = [list(c) for c in concepts_per_item]
        if getattr(self.text_encoder, "t5_many", None) is None:
            cons = [torch.stack([self.t5(c)[0, 0, :] for c in cs]).unsqueeze(0) for cs in concepts_per_item]
        else:
            _, con_vecs = self._t5_with_concepts([], concepts_per_item)
            cons = [torch.stack([con_vecs[c] for c in cs]).unsqueeze(0) for cs in concepts_per_item]
        return [(con, sampling.zero_ids(con.shape[1], con.device, 1)) for con in cons]

    def decode(self, x: torch.Tensor, height: int, width: int):
        """unpack + VAE decode + PIL (image_generator.py:189-204); without an autoencoder the unpacked
        latent is returned as a numpy array."""
        return self.decode_many(x, height, width)[0]

    def decode_many(self, x: torch.Tensor, height: int, width: int) -> list:
        """``decode`` for the B items of ``x``: one image (or latent array) per item.  The HIP autoencoder makes the
        bytes on the device (``AutoEncoder.decode_pixels``) and only they come back; an injected object that has
        ``decode`` alone goes the reference's way through an fp32 image."""
        lat = sampling.unpack(x.float(), height, width)
        if self.ae is None:
            return [lat[k].cpu().numpy() for k in range(lat.shape[0])]
        import PIL.Image
        if hasattr(self.ae, "decode_pixels"):
            pix = self.ae.decode_pixels(lat.to(torch.float32)).cpu().numpy()
        else:
            img = self.ae.decode(lat.to(torch.float32)).clamp(-1, 1).permute(0, 2, 3, 1)
            pix = (127.5 * (img + 1.0)).cpu().byte().numpy()
        return [PIL.Image.fromarray(pix[k]) for k in range(pix.shape[0])]

    def decode_pixels(self, x: torch.Tensor, height: int, width: int) -> torch.Tensor:
        """The bytes ``decode_many`` makes its images from, still on the device: uint8 [B, height, width, 3].  Needs the
        HIP autoencoder (``AutoEncoder.decode_pixels``)."""
        if self.ae is None or not hasattr(self.ae, "decode_pixels"):
            raise ValueError("decode_pixels needs the HIP autoencoder (autoencoder=\"synthetic\" or a .safetensors path)")
        return self.ae.decode_pixels(sampling.unpack(x.float(), height, width).to(torch.float32))

    @torch.no_grad()  # (the reference uses inference_mode; the resident workspace is reused across calls)
    @on_own_device
    def generate_image(self, width, height, num_steps, guidance, seed, prompt, concepts, init_image=None,
                       image2image_strength=0.0, add_sampling_metadata=True, restrict_clip_guidance=False,
                       joint_attention_kwargs=None, latent=None):
        """image_generator.py:87-205.  ``latent`` overrides get_noise (device RNG differs per platform)."""
        seed = int(seed)
        if seed == -1:
            seed = torch.Generator(device="cpu").seed()
        t0 = time.perf_counter()
        x = latent if latent is not None else sampling.get_noise(1, height, width, self.device, torch.bfloat16, seed)
        x = x.to(self.device, torch.bfloat16)
        timesteps = sampling.get_schedule(num_steps, x.shape[-1] * x.shape[-2] // 4, shift=(not self.is_schnell))
        if init_image is not None:  # image-to-image start (:121-158)
            t_idx = int((1 - image2image_strength) * num_steps)
            t = timesteps[t_idx]
            timesteps = timesteps[t_idx:]
            x = (t * x.float() + (1.0 - t) * init_image.to(self.device).float()).to(torch.bfloat16)
        txt, vec, con, con_ids, con_vec = self.embed("" if restrict_clip_guidance else prompt, concepts)
        if restrict_clip_guidance:
            txt = self.t5(prompt)
        inp = sampling.prepare_from_embeddings(x, txt, vec)
        x, _, concept_attention_dict = sampling.denoise(
            self.model, **inp, timesteps=timesteps, guidance=guidance, concepts=con, concept_ids=con_ids,
            concept_vec=con_vec, joint_attention_kwargs=joint_attention_kwargs)
        img = self.decode(x, height, width)
        self.last_seconds = time.perf_counter() - t0
        return img, concept_attention_dict
