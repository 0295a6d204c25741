"""Host-side mirror of the reference's operator interface for this path, on top of the C ABI.

  HipInferenceModel.forward_initial / forward_step / clear_cache / stop_token_ids
      == trait InferenceModel                (/root/reference/src/models/common/mod.rs:25-45)
  generate_generic(...)                      == generate_generic with Sampling::ArgMax when temperature < 1e-7
                                             (/root/reference/src/models/common/generate.rs:70-159, sample.rs:7-37)
Same names, same argument meaning, errors raised as exceptions where the reference returns Err(anyhow!).
Everything numeric happens inside libaha_hip.so; this file only marshals buffers.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import MmInput, ModelDesc, TensorView, check, lib
from .configs import Qwen3ASRConfig, Qwen3Config, Qwen3VLConfig

_DT = {torch.bfloat16: _lib.AHA_BF16, torch.float16: _lib.AHA_F16, torch.float32: _lib.AHA_F32}


class HipContext:
    def __init__(self, device: int = 0):
        self.handle = C.c_void_p()
        check(lib().aha_hip_init(device, C.byref(self.handle)))
        self.device = device

    def close(self):
        if self.handle:
            lib().aha_hip_shutdown(self.handle)
            self.handle = C.c_void_p()


@dataclass
class MultiModalData:
    """data_vec = [pixel_values, image_grid_thw, pixel_values_video, video_grid_thw, cache_position]
    (qwen3vl/generate.rs:79-101, model.rs:1292-1308)."""
    pixel_values: Optional[torch.Tensor] = None    # (n_patches, C*T*P*P) bf16 or f32, processor row order
    image_grid_thw: Optional[np.ndarray] = None    # (n_images, 3) uint32
    pixel_values_video: Optional[torch.Tensor] = None   # the same for the sampled frames of the videos (process_videos)
    video_grid_thw: Optional[np.ndarray] = None    # (n_videos, 3) uint32, t = temporal patches (frame pairs)
    # Qwen3-ASR: data_vec = [input_features] (qwen3_asr/generate.rs:100-125): log-mel (128, F) f32, or raw 16 kHz samples
    audio_features: Optional[np.ndarray] = None
    audio_samples: Optional[np.ndarray] = None
    # image-parallel ViT: embeddings already computed (vision_encode, gathered over RCCL): (1+K, n_tokens, H) bf16 on the GPU
    image_embeds: Optional[torch.Tensor] = None


def _mm_input(data: MultiModalData):
    """MultiModalData -> aha_mm_input.  Returns (struct, arrays the struct points into: keep them alive for the call)."""
    mm = MmInput()
    keep = []
    if data.pixel_values is not None:
        pv = data.pixel_values.detach().contiguous()
        if pv.is_cuda:  # produced on torch's stream; the library copies on its own stream
            torch.cuda.current_stream(pv.device).synchronize()
        grid = np.ascontiguousarray(np.asarray(data.image_grid_thw, dtype=np.uint32).reshape(-1, 3))
        keep += [pv, grid]
        mm.pixel_values = pv.data_ptr()
        mm.pixel_dtype = _DT[pv.dtype]
        mm.n_patches = pv.shape[0]
        mm.image_grid_thw = grid.ctypes.data_as(C.POINTER(C.c_uint32))
        mm.n_images = grid.shape[0]
    if data.pixel_values_video is not None:
        pvv = data.pixel_values_video.detach().contiguous()
        if pvv.is_cuda:
            torch.cuda.current_stream(pvv.device).synchronize()
        assert data.pixel_values is None or pvv.dtype == data.pixel_values.dtype, "image and video pixel values share a dtype"
        vgrid = np.ascontiguousarray(np.asarray(data.video_grid_thw, dtype=np.uint32).reshape(-1, 3))
        keep += [pvv, vgrid]
        mm.pixel_values_video = pvv.data_ptr()
        mm.pixel_dtype = _DT[pvv.dtype]
        mm.n_patches_video = pvv.shape[0]
        mm.video_grid_thw = vgrid.ctypes.data_as(C.POINTER(C.c_uint32))
        mm.n_videos = vgrid.shape[0]
    if data.image_embeds is not None:
        ie = data.image_embeds.detach().contiguous()
        assert ie.is_cuda and ie.dtype == torch.bfloat16 and ie.dim() == 3
        torch.cuda.current_stream(ie.device).synchronize()
        grid = np.ascontiguousarray(np.asarray(data.image_grid_thw if data.image_grid_thw is not None else [], dtype=np.uint32).reshape(-1, 3))
        keep += [ie, grid]
        mm.image_embeds = ie.data_ptr()
        mm.n_image_tokens = ie.shape[1]
        mm.image_grid_thw = grid.ctypes.data_as(C.POINTER(C.c_uint32)) if grid.shape[0] else None
        mm.n_images = grid.shape[0]
        if data.video_grid_thw is not None and data.pixel_values_video is None:   # (the grids still drive get_rope_index)
            vgrid = np.ascontiguousarray(np.asarray(data.video_grid_thw, dtype=np.uint32).reshape(-1, 3))
            keep.append(vgrid)
            mm.video_grid_thw = vgrid.ctypes.data_as(C.POINTER(C.c_uint32))
            mm.n_videos = vgrid.shape[0]
    if data.audio_features is not None:
        af = np.ascontiguousarray(np.asarray(data.audio_features, dtype=np.float32))
        keep.append(af)
        mm.audio_features = af.ctypes.data_as(C.POINTER(C.c_float))
        mm.n_frames = af.shape[1]
    if data.audio_samples is not None:
        au = np.ascontiguousarray(np.asarray(data.audio_samples, dtype=np.float32).reshape(-1))
        keep.append(au)
        mm.audio_samples = au.ctypes.data_as(C.POINTER(C.c_float))
        mm.n_samples = au.size
    return mm, keep


def _pack_batch(seqs):
    """A batch's token ids, packed: (ids uint32, lengths uint64)."""
    seqs = [np.asarray(x, dtype=np.uint32).reshape(-1) for x in seqs]
    ids = np.ascontiguousarray(np.concatenate(seqs) if seqs else np.zeros(0, np.uint32))
    return ids, np.ascontiguousarray([s.size for s in seqs], dtype=np.uint64)


def _sampling_array(params, n: int):
    """params (one sampling.SamplingParams, or one per sequence) as the C array of n entries."""
    from .sampling import SamplingParams
    if isinstance(params, SamplingParams):
        params = [params] * n
    if len(params) != n:
        raise ValueError(f"{len(params)} sampling params for {n} prompts")
    return (_lib.SamplingParams * max(n, 1))(*[p.to_c() for p in params])


def _mm_array(data, n: int):
    """data (None, or per prompt a MultiModalData or None) as the C array of n aha_mm_input pointers (None for data None).  Returns
    (array, what its entries point into: keep it alive for the call)."""
    if data is None:
        return None, []
    if len(data) != n:
        raise ValueError(f"{len(data)} MultiModalData entries for {n} prompts")
    keep, mm_arr = [], (C.c_void_p * max(n, 1))()
    for j, d in enumerate(data):
        if d is not None:
            mm, k = _mm_input(d)
            keep += [mm, k]
            mm_arr[j] = C.addressof(mm)
    return mm_arr, keep


def _top_logprobs_array(top_logprobs, n: int):
    """top_logprobs (an int or None for every prompt, or one entry per prompt; None = no logprobs for that prompt) as int32[n + 1]: -1 for
    None, and one trailing pad element so the array is never empty."""
    tops = [top_logprobs] * n if top_logprobs is None or isinstance(top_logprobs, (int, np.integer)) else list(top_logprobs)
    if len(tops) != n:
        raise ValueError(f"{len(tops)} top_logprobs entries for {n} prompts")
    return np.ascontiguousarray(np.asarray([-1 if t is None else int(t) for t in tops] + [0], dtype=np.int32))


def _unpack_logprobs(lp, top, toks, max_new: int):
    """The aha_token_logprobs block of a batch call -> per prompt None (it asked for none) or one _token_logprobs per generated token."""
    return [None if top[j] < 0 else [_token_logprobs(lp[j * int(max_new) + t]) for t in range(len(toks[j]))] for j in range(len(toks))]


def make_desc(cfg, kv_reserve_tokens: int = 0) -> ModelDesc:
    d = ModelDesc()
    if isinstance(cfg, Qwen3VLConfig):
        t, v = cfg.text, cfg.vision
        d.arch = _lib.AHA_ARCH_QWEN3VL
        d.vis_depth, d.vis_hidden_size, d.vis_num_heads = v.depth, v.hidden_size, v.num_heads
        d.vis_intermediate_size, d.vis_in_channels, d.vis_patch_size = v.intermediate_size, v.in_channels, v.patch_size
        d.vis_temporal_patch_size, d.vis_spatial_merge_size = v.temporal_patch_size, v.spatial_merge_size
        d.vis_out_hidden_size, d.vis_num_position_embeddings = v.out_hidden_size, v.num_position_embeddings
        for i, x in enumerate(v.deepstack_visual_indexes):
            d.vis_deepstack_indexes[i] = x
        d.vis_num_deepstack = len(v.deepstack_visual_indexes)
        d.image_token_id, d.video_token_id = cfg.image_token_id, cfg.video_token_id
        d.vision_start_token_id, d.vision_end_token_id = cfg.vision_start_token_id, cfg.vision_end_token_id
        tie = cfg.tie_word_embeddings
    elif isinstance(cfg, Qwen3ASRConfig):
        t, a = cfg.text, cfg.audio
        d.arch = _lib.AHA_ARCH_QWEN3ASR
        d.aud_d_model, d.aud_encoder_layers, d.aud_attention_heads = a.d_model, a.encoder_layers, a.encoder_attention_heads
        d.aud_ffn_dim, d.aud_num_mel_bins, d.aud_downsample_hidden_size = a.encoder_ffn_dim, a.num_mel_bins, a.downsample_hidden_size
        d.aud_output_dim, d.aud_n_window = a.output_dim, a.n_window
        d.audio_token_id = cfg.audio_token_id
        tie = t.tie_word_embeddings
    else:
        t = cfg
        d.arch = _lib.AHA_ARCH_QWEN3
        tie = cfg.tie_word_embeddings
    d.hidden_size, d.intermediate_size, d.num_hidden_layers = t.hidden_size, t.intermediate_size, t.num_hidden_layers
    d.num_attention_heads, d.num_key_value_heads, d.head_dim = t.num_attention_heads, t.num_key_value_heads, t.head_dim
    d.vocab_size = t.vocab_size
    d.rms_norm_eps, d.rope_theta = t.rms_norm_eps, t.rope_theta
    d.tie_word_embeddings = int(tie)
    ms = t.mrope_section or [0, 0, 0]
    for i in range(3):
        d.mrope_section[i] = ms[i]
    d.kv_reserve_tokens = kv_reserve_tokens
    eos = list(t.eos_token_ids)[:8]
    d.n_stop_tokens = len(eos)
    for i, e in enumerate(eos):
        d.stop_tokens[i] = e
    return d


def tp_unique_id() -> bytes:
    """RCCL unique id for aha_hip_tp_init_rccl: rank 0 makes it, every rank of the TP group receives the same bytes."""
    buf = C.create_string_buffer(128)
    check(lib().aha_hip_tp_unique_id(buf))
    return buf.raw


class HipInferenceModel:
    """One model instance on one GPU (== XxxGenerateModel::init's model object, qwen3/generate.rs:22-50)."""

    def __init__(self, cfg, weights: Dict[str, torch.Tensor], ctx: Optional[HipContext] = None, device: int = 0,
                 kv_reserve_tokens: int = 0, tp_rank: int = 0, tp_size: int = 1, allreduce=None,
                 rccl_unique_id: Optional[bytes] = None, reduce_scatter=None, all_gather=None):
        """tp_size > 1 shards the decoder stack (heads / MLP columns) over ranks; every rank passes the FULL weights and
        the library slices them.  The all-reduce is either RCCL (rccl_unique_id: 128 bytes from tp_unique_id(), shared
        by all ranks) or a host callback allreduce(ptr: int, count: int) -> None that sums `count` f32 at device
        pointer `ptr` over ranks in place (the seam a gloo test or another transport plugs into).
        reduce_scatter(ptr, count_per_rank) / all_gather(ptr, bytes_per_rank) (both or neither; in place, semantics in
        include/aha_hip.h aha_hip_set_seq_parallel) switch the prefill to the sequence-parallel form; with RCCL it is on by
        itself."""
        self.cfg = cfg
        self.text_cfg: Qwen3Config = cfg.text if isinstance(cfg, (Qwen3VLConfig, Qwen3ASRConfig)) else cfg
        self._own_ctx = ctx is None
        self.ctx = ctx or HipContext(device)
        self.handle = C.c_void_p()
        desc = make_desc(cfg, kv_reserve_tokens)
        desc.tp_rank, desc.tp_size = tp_rank, tp_size
        views = (TensorView * len(weights))()
        keep = []
        for i, (name, t) in enumerate(weights.items()):
            t = t.detach().contiguous()
            if t.dtype not in _DT:
                raise TypeError(f"{name}: unsupported dtype {t.dtype}")
            keep.append(t)
            views[i].name = name.encode()
            views[i].data = t.data_ptr()
            views[i].dtype = _DT[t.dtype]
            views[i].ndim = t.dim()
            for j, s in enumerate(t.shape):
                views[i].shape[j] = s
            views[i].on_device = int(t.is_cuda)
        if any(t.is_cuda for t in keep):
            torch.cuda.synchronize()
        check(lib().aha_hip_model_create(self.ctx.handle, C.byref(desc), views, len(weights), C.byref(self.handle)))
        del keep
        self._allreduce_c = None
        if rccl_unique_id is not None:
            buf = C.create_string_buffer(bytes(rccl_unique_id), 128)
            check(lib().aha_hip_tp_init_rccl(self.handle, buf))
        elif tp_size > 1 and allreduce is not None:
            def _cb(ptr, count, _user):
                try:
                    allreduce(int(ptr), int(count))
                    return 0
                except Exception:  # noqa: BLE001 -- must not unwind through C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            self._allreduce_c = _lib.ALLREDUCE_FN(_cb)
            check(lib().aha_hip_set_allreduce(self.handle, self._allreduce_c, None))
            if (reduce_scatter is None) != (all_gather is None):
                raise ValueError("pass both reduce_scatter and all_gather, or neither")
            if reduce_scatter is not None:
                def _wrap(fn):
                    def _c(ptr, n, _user):
                        try:
                            fn(int(ptr), int(n))
                            return 0
                        except Exception:  # noqa: BLE001
                            import traceback
                            traceback.print_exc()
                            return 1
                    return _c
                self._rs_c = _lib.REDUCE_SCATTER_FN(_wrap(reduce_scatter))
                self._ag_c = _lib.ALL_GATHER_FN(_wrap(all_gather))
                check(lib().aha_hip_set_seq_parallel(self.handle, self._rs_c, self._ag_c, None))
        self.vocab = self.text_cfg.vocab_size
        self._logits = np.empty(self.vocab, dtype=np.float32)

    def set_context_parallel(self, rank: int, world: int, all_gather=None, rccl_unique_id: Optional[bytes] = None) -> None:
        """Context-parallel prefill (include/aha_hip.h aha_hip_set_context_parallel): this model holds the FULL weights (tp_size 1) and
        owns two row chunks of every prompt of a fresh cache; per layer the ranks all-gather the layer's K / V pages -- over RCCL
        (rccl_unique_id: 128 bytes from tp_unique_id(), the same on every rank) or through the host callback
        all_gather(ptr: int, bytes_per_rank: int) (in place: rank r's slice is its contribution).  After forward_initial every rank holds
        the whole cache and the last position's logits.  world = 1 switches it off."""
        self._cp_ag_c = None
        if all_gather is not None:
            def _c(ptr, n, _user):
                try:
                    all_gather(int(ptr), int(n))
                    return 0
                except Exception:  # noqa: BLE001 -- must not unwind through C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cp_ag_c = _lib.ALL_GATHER_FN(_c)
        check(lib().aha_hip_set_context_parallel(self.handle, rank, world, self._cp_ag_c, None))
        if rccl_unique_id is not None:
            buf = C.create_string_buffer(bytes(rccl_unique_id), 128)
            check(lib().aha_hip_cp_init_rccl(self.handle, buf))

    @classmethod
    def from_pretrained(cls, path: str, ctx: Optional[HipContext] = None, device: int = 0, kv_reserve_tokens: int = 0):
        """== XxxGenerateModel::init(path, device, dtype) minus tokenizer / chat template (qwen3/generate.rs:22-50): the
        native loader reads config.json + generation_config.json, mmaps every *.safetensors file and builds the model."""
        from .checkpoint import config_from_desc, parse_config
        self = cls.__new__(cls)
        self.desc = parse_config(path)
        self.cfg = config_from_desc(self.desc)
        self.text_cfg = self.cfg.text if isinstance(self.cfg, (Qwen3VLConfig, Qwen3ASRConfig)) else self.cfg
        self._own_ctx = ctx is None
        self.ctx = ctx or HipContext(device)
        self.handle = C.c_void_p()
        self._allreduce_c = None
        check(lib().aha_hip_model_load(self.ctx.handle, os.fsencode(path), kv_reserve_tokens, C.byref(self.handle)))
        self.vocab = int(self.desc.vocab_size)
        self._logits = np.empty(self.vocab, dtype=np.float32)
        return self

    # -- InferenceModel ------------------------------------------------------------------------------------------
    def forward_initial(self, input_ids: Sequence[int], seqlen_offset: int, data: Optional[MultiModalData] = None,
                        want_logits: bool = True):
        ids = np.ascontiguousarray(np.asarray(input_ids, dtype=np.uint32).reshape(-1))
        am = C.c_uint32()
        mm_ref, keep = None, None
        if data is not None:
            mm, keep = _mm_input(data)
            mm_ref = C.byref(mm)
        lp = self._logits.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None
        check(lib().aha_hip_forward_initial(self.handle, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size,
                                            seqlen_offset, mm_ref, lp, C.byref(am)))
        return (self._logits.copy() if want_logits else None), int(am.value)

    def forward_step(self, token: int, seqlen_offset: int, want_logits: bool = True):
        am = C.c_uint32()
        lp = self._logits.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None
        check(lib().aha_hip_forward_step(self.handle, int(token), seqlen_offset, lp, C.byref(am)))
        return (self._logits.copy() if want_logits else None), int(am.value)

    def clear_cache(self):
        check(lib().aha_hip_clear_cache(self.handle))

    def stop_token_ids(self) -> List[int]:
        buf = (C.c_uint32 * 8)()
        n = check(lib().aha_hip_stop_token_ids(self.handle, buf, 8))
        return [int(buf[i]) for i in range(n)]

    # -- extensions ----------------------------------------------------------------------------------------------
    def decode_greedy(self, first_token: int, seqlen_offset: int, max_new: int) -> List[int]:
        buf = (C.c_uint32 * max(max_new, 1))()
        n = check(lib().aha_hip_decode_greedy(self.handle, int(first_token), seqlen_offset, max_new, buf))
        return [int(buf[i]) for i in range(n)]

    def sample_candidates(self, context: Sequence[int], repeat_penalty: float, temperature: float, k: int):
        """Device half of sample_and_push (common/generate.rs:70-86): repeat penalty over `context`, then the k largest
        logits of the last forward call -> (values f32[k], indices u32[k], max, sumexp over the whole vocabulary)."""
        ctx = np.ascontiguousarray(np.asarray(context, dtype=np.uint32).reshape(-1))
        n = max(int(k), 1)  # a bad k is reported by the library, not by numpy
        vals = np.empty(n, dtype=np.float32)
        idx = np.empty(n, dtype=np.uint32)
        mx, se = C.c_float(), C.c_float()
        check(lib().aha_hip_sample_candidates(self.handle, ctx.ctypes.data_as(C.POINTER(C.c_uint32)), ctx.size,
                                              float(repeat_penalty), float(temperature), int(k),
                                              vals.ctypes.data_as(C.POINTER(C.c_float)),
                                              idx.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(mx), C.byref(se)))
        return vals, idx, float(mx.value), float(se.value)

    def last_logits(self) -> np.ndarray:
        out = np.empty(self.text_cfg.vocab_size, dtype=np.float32)
        check(lib().aha_hip_last_logits(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def debug_allreduce(self, t: torch.Tensor) -> None:
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        torch.cuda.current_stream(t.device).synchronize()
        check(lib().aha_hip_debug_allreduce(self.handle, t.data_ptr(), t.numel()))

    # -- TextEmbedding / TextRerank (common/embedding.rs:7-9, common/reranker.rs:5-7) ------------------------------------
    def embed_one(self, input_ids: Sequence[int]) -> np.ndarray:
        """Qwen3Embedding::embed_one after tokenisation (qwen3_embedding/mod.rs:50-64): L2-normalised last hidden state."""
        ids = np.ascontiguousarray(np.asarray(input_ids, dtype=np.uint32).reshape(-1))
        out = np.empty(self.text_cfg.hidden_size, dtype=np.float32)
        check(lib().aha_hip_embed(self.handle, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size,
                                  out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def embed_batch(self, inputs: Sequence[Sequence[int]], max_tokens_per_pass: int = 0) -> np.ndarray:
        """embed_one of every sequence, run as packed prefills (aha_hip_embed_batch): (len(inputs), hidden) float32.
        max_tokens_per_pass = 0 takes the library default; a longer sequence still runs whole, alone in its pass."""
        ids, lens = _pack_batch(inputs)
        out = np.empty((lens.size, self.text_cfg.hidden_size), dtype=np.float32)
        check(lib().aha_hip_embed_batch(self.handle, ids.ctypes.data, lens.ctypes.data, lens.size, int(max_tokens_per_pass),
                                        out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def _generate_batch(self, entry, prompts, extra, max_new: int, max_tokens_per_pass: int, logits: Optional[str]):
        """The packing and unpacking of the generate_batch* wrappers: entry(handle, ids, lens, n, *extra, max_new, max_tokens_per_pass,
        tokens, n_out, logits).  logits: None, "last" = (n, vocab) or "step" = (n, max_new, vocab) float32, returned after the token lists."""
        ids, lens = _pack_batch(prompts)
        n, width, V = lens.size, max(int(max_new), 1), self.text_cfg.vocab_size
        toks = np.zeros((n, width), dtype=np.uint32)
        n_out = np.zeros(n, dtype=np.uint64)
        lg = None if logits is None else np.empty((n, V), np.float32) if logits == "last" else np.zeros((n, width, V), np.float32)
        check(entry(self.handle, ids.ctypes.data, lens.ctypes.data, n, *extra, int(max_new), int(max_tokens_per_pass), toks.ctypes.data,
                    n_out.ctypes.data, None if lg is None else lg.ctypes.data))
        out = [[int(t) for t in toks[j, :int(n_out[j])]] for j in range(n)]
        return out if lg is None else (out, lg)

    def generate_batch(self, prompts: Sequence[Sequence[int]], max_new: int, max_tokens_per_pass: int = 0, want_logits: bool = False):
        """Greedy generation of every prompt at once (aha_hip_generate_batch): per prompt, the tokens generate_generic(device_loop=True)
        yields for it alone at temperature 0.  Returns a list of token lists, and with want_logits also the (len(prompts), vocab) float32
        logits that chose each prompt's last token."""
        return self._generate_batch(lib().aha_hip_generate_batch, prompts, (), max_new, max_tokens_per_pass, "last" if want_logits else None)

    def generate_batch_sampled(self, prompts: Sequence[Sequence[int]], params, max_new: int, max_tokens_per_pass: int = 0,
                               want_step_logits: bool = False):
        """Sampled generation of every prompt at once (aha_hip_generate_batch_sampled): per prompt, the tokens generate_generic_sampled
        yields for it alone with params[j] (a sampling.SamplingParams each, or one for all prompts).  Returns a list of token lists, and
        with want_step_logits also the (len(prompts), max_new, vocab) float32 logits before the penalty that chose each token (rows past
        a sequence's length are zero)."""
        return self._generate_batch(lib().aha_hip_generate_batch_sampled, prompts, (_sampling_array(params, len(prompts)),), max_new,
                                    max_tokens_per_pass, "step" if want_step_logits else None)

    def generate_batch_mm(self, prompts: Sequence[Sequence[int]], data, max_new: int, params=None, max_tokens_per_pass: int = 0,
                          want_step_logits: bool = False):
        """Generation of every request at once, with its images / videos or its audio clip (aha_hip_generate_batch_mm): data[j] is
        request j's MultiModalData -- pixel values and grids (no image_embeds) on a Qwen3-VL model, audio_samples or audio_features on a
        Qwen3-ASR model (samples win if both are set) -- or None for a text request; data itself may be None.
        params: None = every request greedy, else a sampling.SamplingParams per request (or one for all).  Per request, the tokens
        generate_generic yields for it alone with its data.  Returns a list of token lists, and with want_step_logits also the
        (len(prompts), max_new, vocab) float32 logits that chose each token (rows past a sequence's length are zero)."""
        n = len(prompts)
        mm_arr, keep = _mm_array(data, n)
        cp = None if params is None else _sampling_array(params, n)
        return self._generate_batch(lib().aha_hip_generate_batch_mm, prompts, (mm_arr, cp), max_new, max_tokens_per_pass,
                                    "step" if want_step_logits else None)

    def generate_batch_logprobs(self, prompts: Sequence[Sequence[int]], max_new: int, top_logprobs, data=None, params=None,
                                max_tokens_per_pass: int = 0, want_step_logits: bool = False):
        """generate_batch_mm plus per-token log-probabilities (aha_hip_generate_batch_logprobs): the same tokens and step logits, bit for
        bit.  top_logprobs: an int (0..20) for every prompt, or one entry per prompt with None = no logprobs for that prompt.  The
        log-probabilities are those of the model's own distribution over the step's logits (temperature 1, before the repeat penalty),
        whatever the sampler.  Returns (token lists, logprobs[, step logits]): logprobs[j] is None for a prompt that asked for none, else
        per generated token (logprob, [(id, logprob), ...]) with the top_logprobs most likely tokens, most likely first."""
        n = len(prompts)
        mm_arr, keep = _mm_array(data, n)
        top = _top_logprobs_array(top_logprobs, n)
        cp = None if params is None else _sampling_array(params, n)
        lp = (_lib.TokenLogprobs * max(n * max(int(max_new), 1), 1))()

        def entry(handle, ids, lens, n_, mm_, cp_, mx, pas, toks, n_out, lg):
            return lib().aha_hip_generate_batch_logprobs(handle, ids, lens, n_, mm_, cp_, top.ctypes.data, mx, pas, toks, n_out, lg, lp)
        res = self._generate_batch(entry, prompts, (mm_arr, cp), max_new, max_tokens_per_pass, "step" if want_step_logits else None)
        toks = res[0] if want_step_logits else res
        out = _unpack_logprobs(lp, top, toks, max_new)
        return (toks, out, res[1]) if want_step_logits else (toks, out)

    def generate_batch_adjusted(self, prompts: Sequence[Sequence[int]], max_new: int, params=None, top_logprobs=None, data=None,
                                max_tokens_per_pass: int = 0, want_step_logits: bool = False):
        """generate_batch_logprobs whose sampling.SamplingParams also carry logit_bias / presence_penalty / frequency_penalty
        (aha_hip_generate_batch_adjusted; include/aha_hip.h states the definition).  params: None = greedy without any adjust, one
        SamplingParams for all, or one per prompt.  top_logprobs: None = no logprobs at all, else as generate_batch_logprobs.  Returns
        (token lists, logprobs or None[, step logits])."""
        return self._generate_batch_adjusted(prompts, max_new, params, top_logprobs, data, max_tokens_per_pass, want_step_logits, None)

    def generate_batch_masked(self, prompts: Sequence[Sequence[int]], max_new: int, constraint=None, params=None, top_logprobs=None,
                              data=None, max_tokens_per_pass: int = 0, want_step_logits: bool = False):
        """generate_batch_adjusted under a per-step allowed-token mask (aha_hip_generate_batch_masked; include/aha_hip.h states the
        definition).  constraint: a callable (seq, generated) -> packed words (guided.pack_mask) or None, asked once per live prompt per
        step -- generated is the prompt's token list so far, empty for the first token -- while the step's device work runs; None means
        the step is unmasked, a negative int fails the call (AHA_ERR_STATE).  guided.ChoiceConstraint is one; constraint None is generate_batch_adjusted.  An exception the
        constraint raises ends the call (the cache is cleared) and is raised again here."""
        return self._generate_batch_adjusted(prompts, max_new, params, top_logprobs, data, max_tokens_per_pass, want_step_logits, constraint)

    def _generate_batch_adjusted(self, prompts, max_new, params, top_logprobs, data, max_tokens_per_pass, want_step_logits, constraint):
        n = len(prompts)
        mm_arr, keep = _mm_array(data, n)
        from .sampling import SamplingParams
        plist = None if params is None else [params] * n if isinstance(params, SamplingParams) else list(params)
        cp = None if plist is None else _sampling_array(plist, n)
        adj = None
        if plist is not None:
            adj = (_lib.LogitAdjust * max(n, 1))()
            for j, p in enumerate(plist):
                adj[j], k = p.adjust_to_c()
                keep.append(k)
        top = None if top_logprobs is None else _top_logprobs_array(top_logprobs, n)
        lp = None if top is None else (_lib.TokenLogprobs * max(n * max(int(max_new), 1), 1))()

        raised = []

        def on_mask(user, seq, generated, n_generated, words, n_words):   # aha_token_mask_fn
            try:
                got = constraint(int(seq), np.ctypeslib.as_array(generated, shape=(n_generated,)).tolist() if n_generated else [])
                if got is None:
                    return 0
                if isinstance(got, (int, np.integer)) and got < 0:   # the C callback's own failure code: AHA_ERR_STATE names the prompt
                    return int(got)
                w = np.ascontiguousarray(got, dtype=np.uint32).reshape(-1)
                if w.size != n_words:
                    raise ValueError(f"the constraint returned {w.size} words for prompt {seq}, the vocabulary needs {n_words}")
                C.memmove(words, w.ctypes.data, 4 * n_words)
                return 1
            except BaseException as e:   # (nothing may propagate through the C frames)
                raised.append(e)
                return -1
        cb = None if constraint is None else _lib.TOKEN_MASK_FN(on_mask)

        def entry(handle, ids, lens, n_, mm_, cp_, mx, pas, toks, n_out, lg):
            if cb is None:
                return lib().aha_hip_generate_batch_adjusted(handle, ids, lens, n_, mm_, cp_, adj, None if top is None else top.ctypes.data, mx,
                                                             pas, toks, n_out, lg, lp)
            return lib().aha_hip_generate_batch_masked(handle, ids, lens, n_, mm_, cp_, adj, None if top is None else top.ctypes.data, mx, pas,
                                                       C.cast(cb, C.c_void_p), None, toks, n_out, lg, lp)
        try:
            res = self._generate_batch(entry, prompts, (mm_arr, cp), max_new, max_tokens_per_pass, "step" if want_step_logits else None)
        except Exception:
            if raised:
                raise raised[0]
            raise
        toks = res[0] if want_step_logits else res
        out = None if top is None else _unpack_logprobs(lp, top, toks, max_new)
        return (toks, out, res[1]) if want_step_logits else (toks, out)

    def generate_batch_spec(self, prompts: Sequence[Sequence[int]], max_new: int, spec=None, predictions=None, want_logits: bool = False,
                            want_stats: bool = False, max_tokens_per_pass: int = 0):
        """generate_batch with draft-and-verify decoding (aha_hip_generate_batch_spec): the same tokens and logits, bit for bit, in fewer
        decode steps when the drafts are right.  spec: a speculative.SpecConfig (None: its defaults); predictions: None, or per prompt
        its predicted output (a token list; None or empty = no prediction for that prompt) -- drafts come from the prediction first, then
        from n-gram lookup in the prompt and the generated text (speculative.propose).  Returns the token lists; with want_logits also the
        (len(prompts), vocab) float32 logits that chose each prompt's last token; with want_stats also a dict: "proposed" / "accepted"
        (per prompt draft tokens run / kept) and "stats" (a speculative.SpecStats over the call)."""
        from .speculative import SpecConfig, SpecStats
        from ._lib import SpecConfig as CSpecConfig, SpecStats as CSpecStats
        spec = spec or SpecConfig()
        cspec = CSpecConfig(int(spec.max_draft), int(spec.ngram_min), int(spec.ngram_max))
        n = len(prompts)
        pp = pl = None
        if predictions is not None:
            if len(predictions) != n:
                raise ValueError(f"{len(predictions)} predictions for {n} prompts")
            pl = np.asarray([0 if p is None else len(p) for p in predictions], dtype=np.uint64)
            flat = [int(t) for p in predictions if p is not None for t in p]
            pp = np.ascontiguousarray(np.asarray(flat + [0], dtype=np.uint32))   # never a null pointer, even when every prediction is empty
        prop, acc, st = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), CSpecStats()
        extra = (C.byref(cspec), None if pp is None else pp.ctypes.data, None if pl is None else pl.ctypes.data)

        def entry(handle, ids, lens, n_, ex0, ex1, ex2, mx, pas, toks, n_out, lg):
            return lib().aha_hip_generate_batch_spec(handle, ids, lens, n_, mx, pas, ex0, ex1, ex2, toks, n_out, lg, prop.ctypes.data,
                                                     acc.ctypes.data, C.byref(st))
        res = self._generate_batch(entry, prompts, extra, max_new, max_tokens_per_pass, "last" if want_logits else None)
        if not want_stats:
            return res
        info = {"proposed": [int(v) for v in prop[:n]], "accepted": [int(v) for v in acc[:n]],
                "stats": SpecStats(int(st.decode_steps), int(st.rows), int(st.proposed), int(st.accepted))}
        return (*res, info) if want_logits else (res, info)

    def embed_multi(self, inputs: Sequence[Sequence[int]]) -> np.ndarray:
        if len(inputs) == 0:
            raise ValueError("embedding input cannot be empty")  # qwen3_embedding/mod.rs:39-41
        return self.embed_batch(inputs)

    def rerank(self, query_ids: Sequence[int], documents_ids: Sequence[Sequence[int]]) -> np.ndarray:
        """Qwen3Reranker::rerank (qwen3_reranker/mod.rs:23-31): cosine_similarity_no_l2(query, docs) on normalised vectors.
        The query and the documents go through one embed_batch call."""
        if len(documents_ids) == 0:
            raise ValueError("embedding input cannot be empty")  # embed_multi of the documents, qwen3_embedding/mod.rs:39-41
        e = self.embed_batch([query_ids, *documents_ids])
        return (e[:1] @ e[1:].T)[0]

    def cache_len(self) -> int:
        return int(lib().aha_hip_cache_len(self.handle))

    def kv_export(self):
        """aha_hip_kv_export: -> (uint8 tensor on this model's GPU holding [layer][page][local kv head][K | V] blocks, n_tokens,
        rope_delta).  The byte image of this rank's share of the cache -- what crosses the gather after a sharded prefill."""
        need, ntok, delta = C.c_size_t(), C.c_size_t(), C.c_int64()
        check(lib().aha_hip_kv_export(self.handle, None, 0, C.byref(need), C.byref(ntok), C.byref(delta)))
        buf = torch.empty(need.value, dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
        torch.cuda.current_stream(buf.device).synchronize()
        check(lib().aha_hip_kv_export(self.handle, buf.data_ptr(), buf.numel(), None, None, None))
        return buf, int(ntok.value), int(delta.value)

    def kv_import(self, buf: torch.Tensor, src_heads: int, src_head0: int, dst_head0: int, n_heads: int, n_tokens: int, rope_delta: int):
        """aha_hip_kv_import: heads [src_head0, +n_heads) of a packed buffer (src_heads per page) -> this model's heads [dst_head0, ..)."""
        assert buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous()
        torch.cuda.current_stream(buf.device).synchronize()
        check(lib().aha_hip_kv_import(self.handle, buf.data_ptr(), buf.numel(), src_heads, src_head0, dst_head0, n_heads, n_tokens, rope_delta))

    def debug_graph_step(self, replays: int = 50):
        """(us per decode step enqueued launch by launch, us per step replayed as one hipGraph) at the current cache length; clears the cache."""
        a, b = C.c_double(), C.c_double()
        check(lib().aha_hip_debug_graph_step(self.handle, replays, C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_steps_executed(self) -> int:
        return int(lib().aha_hip_debug_steps_executed(self.handle))

    def quantize_weights(self, fmt: str = "mxfp8", lm_head: bool = False) -> None:
        """Quantise the layer matrices (and lm_head with lm_head=True) to MXFP8 in place (aha_hip_model_quantize_weights): the batched decode
        then streams the FP8 copies; every other path reads the dequantised bf16 matrices.  aha_amd/quant.py is the reference quantiser.
        fmt "mxfp4": MXFP4 copies (E2M1 nibbles, 0.53 bytes per weight) for the batched decode and, on the matrices its plan takes
        (debug_fp4_single), the single-sequence decode."""
        formats = {"mxfp8": _lib.AHA_WQ_MXFP8_E4M3, "mxfp4": _lib.AHA_WQ_MXFP4_E2M1}
        if fmt not in formats:
            raise ValueError(f"unknown weight format {fmt!r} (\"mxfp8\", \"mxfp4\")")
        check(lib().aha_hip_model_quantize_weights(self.handle, formats[fmt], _lib.AHA_WQ_LM_HEAD if lm_head else 0))

    @property
    def weight_format(self):
        """None, or ("mxfp8" | "mxfp4", lm_head) as quantize_weights was called."""
        f, fl = C.c_int32(), C.c_uint32()
        check(lib().aha_hip_model_weight_format(self.handle, C.byref(f), C.byref(fl)))
        if f.value == _lib.AHA_WQ_NONE:
            return None
        return ("mxfp4" if f.value == _lib.AHA_WQ_MXFP4_E2M1 else "mxfp8", bool(fl.value & _lib.AHA_WQ_LM_HEAD))

    def debug_fp8_rows(self, on: bool = True) -> None:
        """Test hook: False makes a quantised model's batched decode run the bf16 matvec on the dequantised matrices (the same bits)."""
        check(lib().aha_hip_debug_fp8_rows(self.handle, int(on)))

    def debug_fp8_single(self, on=True) -> None:
        """Test hook: the switch of the single-sequence decode matvec (forward_step, decode_greedy, the generate_generic loops, the last-row
        lm_head of forward_initial).  True / 1 (the default): the FP8 kernel on the matrices whose shape the plan takes (those it measured
        faster on); 2: on every matrix with a copy; False / 0: the bf16 kernel on W'.  The same bits in all three.  Profile class of the FP8
        launches: "gemv_fp8"."""
        check(lib().aha_hip_debug_fp8_single(self.handle, int(on)))

    def debug_pk13_single(self, on=True) -> None:
        """The switch of the single-sequence decode matvec for the exact 13-bit weight copies made when the model was created.  True / 1 (the
        default): the packed kernel on the matrices whose shape its plan takes; 2: on every matrix with a copy; False / 0: the bf16 kernel.
        The same bits in all three; the launches stay in profile class "gemv"."""
        check(lib().aha_hip_debug_pk13_single(self.handle, int(on)))

    def pk13_status(self):
        """{tensor name: "packed", "<n> weights outside the window: packed, rows <list> read from bf16" (a copy whose exception rows the matvec
        computes from the bf16 matrix), or the reason the matrix has no exact 13-bit copy} (aha_hip_pk13_status)."""
        buf = C.create_string_buffer(1 << 16)
        n = lib().aha_hip_pk13_status(self.handle, buf, len(buf))
        if n < 0:
            check(n)
        return dict(line.split("\t", 1) for line in buf.value.decode().splitlines())

    def debug_fp4_single(self, on=True) -> None:
        """Test hook: debug_fp8_single's twin for a model with MXFP4 copies (the FP8 switch reads FP8 copies only).  True / 1 (the default):
        the FP4 kernel on the matrices whose shape its plan takes; 2: on every matrix with a copy; False / 0: the bf16 kernel on W'.  The
        same bits in all three.  Profile class of the FP4 launches: "gemv_fp4"."""
        check(lib().aha_hip_debug_fp4_single(self.handle, int(on)))

    def set_profiling(self, on: bool):
        check(lib().aha_hip_set_profiling(self.handle, int(on)))

    def get_profile(self, kernel_class: str):
        ms, n, b, f = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        check(lib().aha_hip_get_profile(self.handle, kernel_class.encode(), C.byref(ms), C.byref(n), C.byref(b), C.byref(f)))
        return {"ms": ms.value, "launches": n.value, "bytes": b.value, "flops": f.value}

    def debug_attn_decode_form(self) -> int:
        """Form of the fused decode attention in the last decode step: 1 linear (arithmetic page addresses), 0 page table, -1 none yet."""
        return int(lib().aha_hip_debug_attn_decode_form(self.handle))

    def debug_scramble_pages(self, on: bool = True):
        check(lib().aha_hip_debug_scramble_pages(self.handle, int(on)))

    def debug_last_hidden(self) -> np.ndarray:
        out = np.empty(self.text_cfg.hidden_size, dtype=np.float32)
        check(lib().aha_hip_debug_last_hidden(self.handle, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def debug_image_embeds(self, which: int, rows: int) -> np.ndarray:
        out = np.empty((rows, self.text_cfg.hidden_size), dtype=np.float32)
        check(lib().aha_hip_debug_image_embeds(self.handle, which, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def vision_encode(self, data: "MultiModalData") -> torch.Tensor:
        """ViT only (aha_hip_vision_encode): -> (1 + n_deepstack, n_tokens, hidden) bf16 on this model's GPU; the images' tokens
        first, then the videos'."""
        mm = MmInput()
        m2 = self.cfg.vision.spatial_merge_size ** 2
        n_tok = 0
        keep = []
        if data.pixel_values is not None:
            pv = data.pixel_values.detach().contiguous()
            if pv.is_cuda:
                torch.cuda.current_stream(pv.device).synchronize()
            grid = np.ascontiguousarray(np.asarray(data.image_grid_thw, dtype=np.uint32).reshape(-1, 3))
            mm.pixel_values, mm.pixel_dtype, mm.n_patches = pv.data_ptr(), _DT[pv.dtype], pv.shape[0]
            mm.image_grid_thw, mm.n_images = grid.ctypes.data_as(C.POINTER(C.c_uint32)), grid.shape[0]
            n_tok += int(sum(int(g[0]) * int(g[1]) * int(g[2]) for g in grid) // m2)
            keep += [pv, grid]
        if data.pixel_values_video is not None:
            pvv = data.pixel_values_video.detach().contiguous()
            if pvv.is_cuda:
                torch.cuda.current_stream(pvv.device).synchronize()
            vgrid = np.ascontiguousarray(np.asarray(data.video_grid_thw, dtype=np.uint32).reshape(-1, 3))
            mm.pixel_values_video, mm.pixel_dtype, mm.n_patches_video = pvv.data_ptr(), _DT[pvv.dtype], pvv.shape[0]
            mm.video_grid_thw, mm.n_videos = vgrid.ctypes.data_as(C.POINTER(C.c_uint32)), vgrid.shape[0]
            n_tok += int(sum(int(g[0]) * int(g[1]) * int(g[2]) for g in vgrid) // m2)
            keep += [pvv, vgrid]
        k = 1 + len(self.cfg.vision.deepstack_visual_indexes)
        out = torch.empty(k, n_tok, self.text_cfg.hidden_size, dtype=torch.bfloat16, device=f"cuda:{self.ctx.device}")
        nt = C.c_int64()
        check(lib().aha_hip_vision_encode(self.handle, C.byref(mm), out.data_ptr(), C.byref(nt)))
        assert nt.value == n_tok
        return out

    def debug_audio_embeds(self, rows: int) -> np.ndarray:
        out = np.empty((rows, self.text_cfg.hidden_size), dtype=np.float32)
        check(lib().aha_hip_debug_audio_embeds(self.handle, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def close(self):
        if self.handle:
            eng = getattr(self, "_engine", None)
            if eng is not None:   # an engine left open goes first: it owns this model's cache
                eng.close()
            lib().aha_hip_model_destroy(self.handle)
            self.handle = C.c_void_p()
        if self._own_ctx:
            self.ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class EngineEvent:
    """One emitted token of a step (aha_engine_event): flags are AHA_ENGINE_EV_* bits; a cancellation has token None."""
    req_id: int
    token: Optional[int]
    first: bool
    stop: bool
    length: bool
    cancelled: bool

    @property
    def finished(self) -> bool:
        return self.stop or self.length or self.cancelled


def _token_logprobs(e):
    """One aha_token_logprobs -> (logprob, [(id, logprob), ...]); None for an entry whose request asked for none (n_top = -1)."""
    if e.n_top < 0:
        return None
    return float(e.logprob), [(int(e.top_ids[i]), float(e.top_logprobs[i])) for i in range(e.n_top)]


class HipEngine:
    """Continuous batching over one model (aha_hip_engine_*): submit requests at any time, step() returns every token emitted in the
    step, cancel() ends a request at the next step.  The engine owns the model's cache while it lives: the model's other generation
    entries raise AHA_ERR_STATE until close().  generate_stream_generic (common/generate.rs:231-368) for many requests at once."""

    def __init__(self, model: HipInferenceModel, max_running: int = 8, kv_pages: int = 256, max_tokens_per_step: int = 0,
                 prefill_chunk: int = 0):
        self.model = model
        cfg = _lib.EngineConfig(max_running, kv_pages, max_tokens_per_step, prefill_chunk)
        self.handle = C.c_void_p()
        check(lib().aha_hip_engine_create(model.handle, C.byref(cfg), C.byref(self.handle)))
        model._engine = self
        self.max_running = int(max_running)
        self._keep: Dict[int, list] = {}      # per request: the arrays its aha_mm_input points into, until its first token
        self._streams: Dict[int, List[int]] = {}
        self._done: Dict[int, bool] = {}

    def submit(self, input_ids: Sequence[int], max_new: int, params=None, data: Optional[MultiModalData] = None,
               top_logprobs: Optional[int] = None, mask=None, spec=None, prediction: Optional[Sequence[int]] = None) -> int:
        """Queue one request; returns its id.  params: None = greedy, else a sampling.SamplingParams; data: its MultiModalData;
        top_logprobs: None, or 0..20 = report every token's log-probability and that many alternatives (step(want_logprobs=True));
        mask: None, or the packed allowed-token words (guided.pack_mask) that govern its tokens from the first one until set_mask.
        spec: None, or a speculative.SpecConfig = a greedy draft-and-verify request (aha_hip_engine_submit_spec) with its predicted
        output `prediction` (None: prompt lookup only); it takes no params, top_logprobs or mask."""
        ids = np.ascontiguousarray(np.asarray(input_ids, dtype=np.uint32).reshape(-1))
        keep = [ids]
        mm_p = None
        if data is not None:
            mm, k = _mm_input(data)
            keep += [mm, k]
            mm_p = C.byref(mm)
        if spec is not None and (params is not None or top_logprobs is not None or mask is not None):
            raise ValueError("a draft-and-verify request is greedy: no params, top_logprobs or mask")
        if spec is None and prediction is not None:
            raise ValueError("a prediction needs a spec")
        cp = None if params is None else C.byref(params.to_c())
        rid = C.c_uint64()
        head, top = (self.handle, ids.ctypes.data, ids.size, mm_p, cp), -1 if top_logprobs is None else int(top_logprobs)
        adj_p = None
        if params is not None and getattr(params, "adjust_active", False):   # logit_bias / presence / frequency: the arrays are copied
            adj, k = params.adjust_to_c()
            adj_p = C.byref(adj)
        # the entry: spec -> _spec, mask -> _masked, an active adjust -> _adjusted, top_logprobs -> _logprobs, otherwise the plain one
        if spec is not None:
            cs = _lib.SpecConfig(spec.max_draft, spec.ngram_min, spec.ngram_max)
            pred = np.ascontiguousarray(np.asarray([] if prediction is None else prediction, dtype=np.uint32).reshape(-1))
            rc = lib().aha_hip_engine_submit_spec(*head[:4], int(max_new), C.byref(cs), pred.ctypes.data if pred.size else None, pred.size,
                                                  C.byref(rid))
        elif mask is not None:
            words = np.ascontiguousarray(mask, dtype=np.uint32).reshape(-1)
            rc = lib().aha_hip_engine_submit_masked(*head, adj_p, words.ctypes.data, words.size, int(max_new), top, C.byref(rid))
        elif adj_p is not None:
            rc = lib().aha_hip_engine_submit_adjusted(*head, adj_p, int(max_new), top, C.byref(rid))
        elif top_logprobs is not None:
            rc = lib().aha_hip_engine_submit_logprobs(*head, int(max_new), top, C.byref(rid))
        else:
            rc = lib().aha_hip_engine_submit(*head, int(max_new), C.byref(rid))
        check(rc)
        self._keep[rid.value] = keep
        self._streams[rid.value] = []
        self._done[rid.value] = False
        return rid.value

    def set_mask(self, req_id: int, mask) -> None:
        """Replace the allowed-token mask of a waiting or running request (aha_hip_engine_set_mask): packed words (guided.pack_mask), or
        None to clear it.  It stays until it is replaced and acts from the next token the request samples."""
        if mask is None:
            check(lib().aha_hip_engine_set_mask(self.handle, int(req_id), None, 0))
            return
        words = np.ascontiguousarray(mask, dtype=np.uint32).reshape(-1)
        check(lib().aha_hip_engine_set_mask(self.handle, int(req_id), words.ctypes.data, words.size))

    def cancel(self, req_id: int) -> None:
        check(lib().aha_hip_engine_cancel(self.handle, int(req_id)))

    def step(self, want_logits: bool = False, want_logprobs: bool = False):
        """One engine step: a list of EngineEvent (and with want_logits the (len(events), vocab) float32 logits that chose each token;
        with want_logprobs, after them, one entry per event: (logprob, [(id, logprob), ...]), or None for a cancellation or a request
        submitted without top_logprobs)."""
        cap = int(lib().aha_hip_engine_max_events(self.handle))
        evs = (_lib.EngineEvent * cap)()
        n = C.c_size_t()
        lg = np.zeros((cap, self.model.text_cfg.vocab_size), np.float32) if want_logits else None
        lp = (_lib.TokenLogprobs * cap)() if want_logprobs else None
        if lp is None:
            check(lib().aha_hip_engine_step(self.handle, evs, cap, C.byref(n), None if lg is None else lg.ctypes.data))
        else:
            check(lib().aha_hip_engine_step_logprobs(self.handle, evs, cap, C.byref(n), None if lg is None else lg.ctypes.data, lp))
        out = []
        for i in range(n.value):
            e = evs[i]
            f = int(e.flags)
            ev = EngineEvent(int(e.req_id), None if f & _lib.AHA_ENGINE_EV_CANCELLED else int(e.token), bool(f & _lib.AHA_ENGINE_EV_FIRST),
                             bool(f & _lib.AHA_ENGINE_EV_STOP), bool(f & _lib.AHA_ENGINE_EV_LENGTH), bool(f & _lib.AHA_ENGINE_EV_CANCELLED))
            if ev.first or ev.cancelled:
                self._keep.pop(ev.req_id, None)
            if ev.token is not None and ev.req_id in self._streams:
                self._streams[ev.req_id].append(ev.token)
            if ev.finished and ev.req_id in self._done:
                self._done[ev.req_id] = True
            out.append(ev)
        if lp is None:
            return out if lg is None else (out, lg[:n.value])
        lps = [_token_logprobs(lp[i]) for i in range(n.value)]
        return (out, lps) if lg is None else (out, lg[:n.value], lps)

    def stats(self) -> Dict[str, int]:
        st = _lib.EngineStats()
        check(lib().aha_hip_engine_stats(self.handle, C.byref(st)))
        return {"waiting": st.waiting, "running": st.running, "free_pages": st.free_pages, "total_pages": st.total_pages}

    def max_events(self) -> int:
        """The cap the next step needs (aha_hip_engine_max_events): max_running, or the row budget of max_running while a request that
        may draft is waiting or running, plus pending cancellations."""
        return int(lib().aha_hip_engine_max_events(self.handle))

    def spec_stats(self):
        """speculative.SpecStats over the engine's life (aha_hip_engine_spec_stats)."""
        from .speculative import SpecStats
        st = _lib.SpecStats()
        check(lib().aha_hip_engine_spec_stats(self.handle, C.byref(st)))
        return SpecStats(int(st.decode_steps), int(st.rows), int(st.proposed), int(st.accepted))

    def request_spec(self, req_id: int):
        """(proposed, accepted) draft tokens of a running request, or of one the most recent step ended (aha_hip_engine_request_spec)."""
        p, a = C.c_size_t(), C.c_size_t()
        check(lib().aha_hip_engine_request_spec(self.handle, int(req_id), C.byref(p), C.byref(a)))
        return int(p.value), int(a.value)

    def tokens(self, req_id: int) -> List[int]:
        """The tokens request req_id has streamed so far."""
        return list(self._streams[req_id])

    def forget(self, req_id: int) -> None:
        """Drop a finished request's record (its tokens, its state): a long-lived engine keeps none of them otherwise."""
        if not self._done.get(req_id, True):
            raise ValueError(f"request {req_id} has not finished")
        self._streams.pop(req_id, None)
        self._done.pop(req_id, None)

    def finished(self, req_id: int) -> bool:
        return self._done[req_id]

    def stream(self, req_id: int):
        """Per-request token iterator: yields req_id's tokens as steps emit them, stepping the engine (every request advances).  The
        request's record is dropped once the iterator is exhausted (forget)."""
        sent = 0
        while True:
            toks = self._streams[req_id]
            while sent < len(toks):
                yield toks[sent]
                sent += 1
            if self._done[req_id]:
                self.forget(req_id)
                return
            self.step()

    def debug_ctr_base(self, base: int) -> None:
        check(lib().aha_hip_engine_debug_ctr_base(self.handle, int(base) & 0xFFFFFFFF))

    def close(self):
        if self.handle:
            lib().aha_hip_engine_destroy(self.handle)
            self.handle = C.c_void_p()
            if getattr(self.model, "_engine", None) is self:
                self.model._engine = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


@dataclass
class Usage:
    """utils/response_utils.rs:225-255 / params/shared.rs:3-28 timing fields."""
    prompt_tokens: int
    prompt_secs: float
    completion_tokens: int
    completion_secs: float
    # params/shared.rs:58-63 (CompletionTokensDetails): filled only by generate_generic_batch_spec
    accepted_prediction_tokens: Optional[int] = None
    rejected_prediction_tokens: Optional[int] = None

    @property
    def completion_tps(self) -> float:
        return self.completion_tokens / self.completion_secs if self.completion_secs > 0 else float("nan")


def generate_generic(model: HipInferenceModel, input_ids: Sequence[int], max_tokens: int,
                     data: Optional[MultiModalData] = None, device_loop: bool = False):
    """generate_generic (common/generate.rs:115-159) with temperature 0 => Sampling::ArgMax (sample.rs:13-37).

    Returns (generated token ids, Usage).  ``device_loop`` uses the aha_hip_decode_greedy extension for the decode
    loop (no per-token host round trip); the token sequence is identical by construction.
    """
    eos = set(model.stop_token_ids())
    generated: List[int] = []
    seqlen_offset, seq_len = 0, len(input_ids)
    t0 = time.perf_counter()
    _, tok = model.forward_initial(input_ids, seqlen_offset, data, want_logits=False)
    generated.append(tok)
    prompt_secs = time.perf_counter() - t0
    t0 = time.perf_counter()
    if device_loop and max_tokens > 1:
        seqlen_offset += seq_len
        generated += model.decode_greedy(tok, seqlen_offset, max_tokens - 1)
    else:
        for _ in range(1, max_tokens):
            seqlen_offset += seq_len
            seq_len = 1
            _, tok = model.forward_step(tok, seqlen_offset, want_logits=False)
            generated.append(tok)
            if tok in eos:
                break
    completion_secs = time.perf_counter() - t0
    model.clear_cache()
    return generated, Usage(len(input_ids), prompt_secs, len(generated), completion_secs)


def generate_generic_batch(model: HipInferenceModel, prompts: Sequence[Sequence[int]], max_tokens: int, max_tokens_per_pass: int = 0):
    """generate_generic at temperature 0 for many text prompts in one call (HipInferenceModel.generate_batch).  Returns (per-prompt
    generated token ids, Usage over all prompts: prompt / completion token totals; prompt_secs 0 and completion_secs the whole call,
    as prefill and decode are not timed apart)."""
    t0 = time.perf_counter()
    out = model.generate_batch(prompts, max_tokens, max_tokens_per_pass)
    secs = time.perf_counter() - t0
    return out, Usage(sum(len(p) for p in prompts), 0.0, sum(len(o) for o in out), secs)


def generate_generic_batch_sampled(model: HipInferenceModel, prompts: Sequence[Sequence[int]], params, max_tokens: int,
                                   max_tokens_per_pass: int = 0):
    """generate_generic with each prompt's own sampler (sampling.SamplingParams, one per prompt or one for all) in one call
    (HipInferenceModel.generate_batch_sampled).  Returns (per-prompt generated token ids, Usage over all prompts, timed as in
    generate_generic_batch)."""
    t0 = time.perf_counter()
    out = model.generate_batch_sampled(prompts, params, max_tokens, max_tokens_per_pass)
    secs = time.perf_counter() - t0
    return out, Usage(sum(len(p) for p in prompts), 0.0, sum(len(o) for o in out), secs)


def generate_generic_batch_mm(model: HipInferenceModel, prompts: Sequence[Sequence[int]], data, max_tokens: int, params=None,
                              max_tokens_per_pass: int = 0):
    """generate_generic for many requests with their images / videos (data: a MultiModalData or None per prompt) in one call
    (HipInferenceModel.generate_batch_mm); params None = greedy.  Returns (per-prompt generated token ids, Usage over all prompts,
    timed as in generate_generic_batch)."""
    t0 = time.perf_counter()
    out = model.generate_batch_mm(prompts, data, max_tokens, params, max_tokens_per_pass)
    secs = time.perf_counter() - t0
    return out, Usage(sum(len(p) for p in prompts), 0.0, sum(len(o) for o in out), secs)


def generate_generic_batch_spec(model: HipInferenceModel, prompts: Sequence[Sequence[int]], max_tokens: int, spec=None, predictions=None,
                                max_tokens_per_pass: int = 0):
    """generate_generic_batch with draft-and-verify decoding (HipInferenceModel.generate_batch_spec): the same tokens; the Usage also
    carries accepted_prediction_tokens / rejected_prediction_tokens (draft tokens kept / run and dropped, over all prompts)."""
    t0 = time.perf_counter()
    out, info = model.generate_batch_spec(prompts, max_tokens, spec, predictions, want_stats=True, max_tokens_per_pass=max_tokens_per_pass)
    secs = time.perf_counter() - t0
    acc, prop = sum(info["accepted"]), sum(info["proposed"])
    return out, Usage(sum(len(p) for p in prompts), 0.0, sum(len(o) for o in out), secs, acc, prop - acc)
