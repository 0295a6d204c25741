"""Op-level entry points of the C ABI on torch device tensors (torch is only the allocator / stream provider here).

Each function is one kernel family of SURVEY.md section 8a; the parity tests compare them with oracle/ on the same
seeded inputs.  All tensors must live on the GPU and be contiguous bf16 unless stated otherwise.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("op inputs must be contiguous GPU tensors")


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    _chk(x, w)
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1]
    check(lib().aha_hip_rmsnorm(_ptr(x), _ptr(w), _ptr(y), rows, x.shape[-1], eps, _stream()))
    return y


def gemv(W: torch.Tensor, x: torch.Tensor, norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6,
         residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(W, x, norm_w, residual)
    N, K = W.shape
    y = torch.empty(N, dtype=torch.bfloat16, device=x.device)
    check(lib().aha_hip_gemv(_ptr(W), _ptr(x), _ptr(y), N, K, _ptr(norm_w), eps, _ptr(residual), _stream()))
    return y


def gemv_gate_up(Wg: torch.Tensor, Wu: torch.Tensor, x: torch.Tensor, norm_w: Optional[torch.Tensor] = None,
                 eps: float = 1e-6) -> torch.Tensor:
    _chk(Wg, Wu, x, norm_w)
    I, K = Wg.shape
    y = torch.empty(I, dtype=torch.bfloat16, device=x.device)
    check(lib().aha_hip_gemv_gate_up(_ptr(Wg), _ptr(Wu), _ptr(x), _ptr(y), I, K, _ptr(norm_w), eps, _stream()))
    return y


def gemm(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, act: int = _lib.ACT_NONE) -> torch.Tensor:
    _chk(A, W, bias, residual)
    M, K = A.shape
    N = W.shape[0]
    n_out = N // 2 if act == _lib.ACT_SILU_MUL_PAIRS else N
    Cm = torch.empty(M, n_out, dtype=torch.bfloat16, device=A.device)
    check(lib().aha_hip_gemm(_ptr(A), _ptr(W), _ptr(Cm), M, N, K, K, W.shape[1], n_out, _ptr(bias), _ptr(residual),
                             act, _stream()))
    return Cm


def poison_lds(seed: int) -> None:
    """Test tool: seeded garbage into the LDS of every CU, on the current stream (aha_hip_debug_poison_lds)."""
    check(lib().aha_hip_debug_poison_lds(int(seed) & 0xFFFFFFFF, _stream()))


def gemm_plan(tile: int = 0, splitk: int = 0) -> None:
    """Test hook: force the 128 / 256 tile kernel and a split-K factor for the following GEMMs; (0, 0) = automatic."""
    check(lib().aha_hip_debug_gemm_plan(tile, splitk))


def gemm_grouped(A: torch.Tensor, W: torch.Tensor, Cm: torch.Tensor, M: int, groups: int, a_gstride: int, c_gstride: int, c_row0: int,
                 m_total: int, act: int = _lib.ACT_NONE) -> None:
    """Test entry (aha_hip_debug_gemm_grouped): segment g = A rows [g * a_gstride, + M) -> Cm rows [c_row0 + g * c_gstride, + M) < m_total."""
    _chk(A, W, Cm)
    N, K = W.shape
    check(lib().aha_hip_debug_gemm_grouped(_ptr(A), _ptr(W), _ptr(Cm), M, N, K, Cm.shape[1], act, groups, a_gstride, c_gstride, c_row0, m_total,
                                           _stream()))


def attn_variant(smx: int = -1) -> None:
    """Test hook: the prefill attention's score-chain variant (aha_hip_debug_attn_variant); -1 = default."""
    check(lib().aha_hip_debug_attn_variant(smx))


def attn_form(form: int = -1) -> None:
    """Test hook: the prefill attention's kernel form (aha_hip_debug_attn_form): 16, 64, 65 (64 pipelined) or -1 = automatic."""
    check(lib().aha_hip_debug_attn_form(form))


def interleave_gate_up(Wg: torch.Tensor, Wu: torch.Tensor) -> torch.Tensor:
    """The model loader's fused layout: 16-row blocks alternating gate / up (csrc/model.hip upload_gate_up)."""
    I, K = Wg.shape
    return torch.stack([Wg.reshape(I // 16, 16, K), Wu.reshape(I // 16, 16, K)], dim=1).reshape(2 * I, K).contiguous()


def qknorm_rope(qkv: torch.Tensor, q_norm_w: torch.Tensor, k_norm_w: torch.Tensor, pos: torch.Tensor,
                axis_map: torch.Tensor, nh: int, kvh: int, d: int, eps: float, theta: float):
    """qkv (S, (nh+2kvh)*d) bf16; pos (3,S) int32; axis_map (d/2) int32 -> q (S,nh*d), k (S,kvh*d), v (S,kvh*d)."""
    _chk(qkv, q_norm_w, k_norm_w, pos, axis_map)
    S = qkv.shape[0]
    q = torch.empty(S, nh * d, dtype=torch.bfloat16, device=qkv.device)
    k = torch.empty(S, kvh * d, dtype=torch.bfloat16, device=qkv.device)
    v = torch.empty(S, kvh * d, dtype=torch.bfloat16, device=qkv.device)
    check(lib().aha_hip_qknorm_rope(_ptr(qkv), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(pos), _ptr(axis_map), _ptr(q),
                                    _ptr(k), _ptr(v), S, nh, kvh, d, eps, theta, _stream()))
    return q, k, v


def attn_decode(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nh: int, kvh: int, d: int,
                scale: Optional[float] = None) -> torch.Tensor:
    """q (nh*d); k, v (L, kvh*d) token-major -> o (nh*d).  The three-launch fallback (attn_decode_kernel + combine), which the model runs
    only with AHA_DECODE_FUSED=0; the default decode kernel is the fused one behind attn_decode_batch / debug_attn_decode_fused
    (tests/test_attn_decode_fused_gpu.py)."""
    _chk(q, k, v)
    L = k.shape[0]
    scale = bf16_scale(d) if scale is None else scale
    o = torch.empty(nh * d, dtype=torch.bfloat16, device=q.device)
    check(lib().aha_hip_attn_decode(_ptr(q), _ptr(k), _ptr(v), _ptr(o), nh, kvh, d, L, scale, _stream()))
    return o


def attn_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nh: int, kvh: int, d: int, kv_offset: int = 0,
                 causal: bool = True, scale: Optional[float] = None) -> torch.Tensor:
    """q (S, nh*d); k, v (L, kvh*d) token-major, L = kv_offset + S when causal -> o (S, nh*d)."""
    _chk(q, k, v)
    S, L = q.shape[0], k.shape[0]
    scale = bf16_scale(d) if scale is None else scale
    o = torch.empty(S, nh * d, dtype=torch.bfloat16, device=q.device)
    check(lib().aha_hip_attn_prefill(_ptr(q), _ptr(k), _ptr(v), _ptr(o), S, L, nh, kvh, d, kv_offset, int(causal),
                                     scale, _stream()))
    return o


def attn_prefill_segs(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nh: int, kvh: int, segs, with_kv0: bool = True,
                      scale: Optional[float] = None) -> torch.Tensor:
    """Test entry (aha_hip_debug_attn_prefill_segs): segs = [(len, kv0), ...]; q (sum len, nh*128) packed in segment order; k, v
    (sum (kv0 + len), kvh*128) every segment's cache back to back.  Causal, row i of a segment at cache position kv0 + i."""
    _chk(q, k, v)
    scale = bf16_scale(128) if scale is None else scale
    o = torch.empty(q.shape[0], nh * 128, dtype=torch.bfloat16, device=q.device)
    flat = (C.c_int32 * (2 * len(segs)))(*[int(x) for sg in segs for x in sg])
    check(lib().aha_hip_debug_attn_prefill_segs(_ptr(q), _ptr(k), _ptr(v), _ptr(o), nh, kvh, flat, len(segs), int(with_kv0), scale,
                                                _stream()))
    return o


ROPE_FORM_TABLE, ROPE_FORM_NO_TABLE, ROPE_FORM_DEVICE_START, ROPE_FORM_PACKED = 0, 1, 2, 3


def debug_prefill_rope(qkv: torch.Tensor, q_norm_w: torch.Tensor, k_norm_w: torch.Tensor, pos: torch.Tensor, axis_map: torch.Tensor,
                       inv_freq: torch.Tensor, page_ptrs: torch.Tensor, nh: int, kvh: int, eps: float, form: int = ROPE_FORM_TABLE,
                       kv_start: int = 0, skip_q: bool = False, row_slot=None, page_rows=None):
    """Test entry (aha_hip_debug_prefill_rope): the prefill's rope table, then its q/k-norm + RoPE + paged KV write, in the form the model
    (ROPE_FORM_TABLE), the in-place-angle A/B (NO_TABLE), the device-scalar path (DEVICE_START) or a packed pass (PACKED: row_slot (S),
    page_rows (n_pages, 2) host ints) launches it.  qkv (S, (nh+2kvh)*128) bf16, pos (3, S) int32, axis_map (64) int32, inv_freq (64) f32,
    page_ptrs (P,) int64 device page addresses into a pool of the caller's.  -> (rope_tab (S, 128) bf16, q (S, nh*128) bf16; with skip_q
    the kernel leaves q as allocated: zeros)."""
    _chk(qkv, q_norm_w, k_norm_w, pos, axis_map, inv_freq, page_ptrs)
    assert pos.dtype == torch.int32 and axis_map.dtype == torch.int32 and inv_freq.dtype == torch.float32 and page_ptrs.dtype == torch.int64
    S = qkv.shape[0]
    assert tuple(pos.shape) == (3, S) and axis_map.numel() == 64 and inv_freq.numel() == 64 and qkv.shape[1] == (nh + 2 * kvh) * 128
    tab = torch.empty(S, 128, dtype=torch.bfloat16, device=qkv.device)
    q = torch.zeros(S, nh * 128, dtype=torch.bfloat16, device=qkv.device)
    slot = prow = None
    n_pages = 0
    if form == ROPE_FORM_PACKED:
        slot = np.ascontiguousarray(np.asarray(row_slot, dtype=np.int32).reshape(S))
        prow = np.ascontiguousarray(np.asarray(page_rows, dtype=np.int32).reshape(-1, 2))
        n_pages = prow.shape[0]
    check(lib().aha_hip_debug_prefill_rope(_ptr(qkv), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(pos), _ptr(axis_map), _ptr(inv_freq), _ptr(page_ptrs),
                                           page_ptrs.numel(), S, nh, kvh, 128, eps, int(form), int(kv_start), int(bool(skip_q)),
                                           None if slot is None else slot.ctypes.data, None if prow is None else prow.ctypes.data, n_pages,
                                           _ptr(tab), _ptr(q), _stream()))
    return tab, q


def debug_prefill_attn_qfuse(qkv: torch.Tensor, q_norm_w: torch.Tensor, rope_tab: torch.Tensor, page_ptrs: torch.Tensor, nh: int, kvh: int,
                             eps: float, kv_offset: int = 0, kv_total: int = 0, seg2=None, segs=None, with_kv0: bool = False,
                             scale: Optional[float] = None) -> torch.Tensor:
    """Test entry (aha_hip_debug_prefill_attn_qfuse): the prefill attention norming + rotating the RAW q heads of qkv in its Q load, over the
    pages debug_prefill_rope wrote.  One sequence: rows at cache positions kv_offset .. of kv_total tokens; seg2 = (S2, kv_offset2,
    kv_total2): the last S2 rows of qkv are a second causal segment of the same launch.  Packed: segs = [(len, page0, kv0), ...].
    -> o (rows, nh*128) bf16.  Raises AhaHipError (AHA_ERR_UNSUPPORTED) where the selected attention form takes no fused Q."""
    _chk(qkv, q_norm_w, rope_tab, page_ptrs)
    assert page_ptrs.dtype == torch.int64 and rope_tab.shape == (qkv.shape[0], 128) and qkv.shape[1] == (nh + 2 * kvh) * 128
    rows = qkv.shape[0]
    scale = bf16_scale(128) if scale is None else scale
    o = torch.empty(rows, nh * 128, dtype=torch.bfloat16, device=qkv.device)
    S2, off2, tot2 = (int(x) for x in seg2) if seg2 else (0, 0, 0)
    flat = (C.c_int32 * (3 * len(segs)))(*[int(x) for sg in segs for x in sg]) if segs else None
    check(lib().aha_hip_debug_prefill_attn_qfuse(_ptr(qkv), _ptr(q_norm_w), _ptr(rope_tab), _ptr(page_ptrs), page_ptrs.numel(), rows - S2, nh, kvh,
                                                 128, eps, scale, int(kv_offset), int(kv_total), S2, off2, tot2, flat, len(segs) if segs else 0,
                                                 int(with_kv0), _ptr(o), _stream()))
    return o


# ---- the vision and audio towers' row kernels (test entries; tests/test_tower_rows_gpu.py) --------------------------------------------------
def debug_layernorm_rows(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None,
                         rows: Optional[int] = None) -> torch.Tensor:
    """Test entry (aha_hip_debug_layernorm_rows): launch_layernorm_rows over the first `rows` rows (default: all) of x (R, dim) bf16 into
    `out` (default: a new tensor)."""
    _chk(x, w, b, out)
    out = torch.empty_like(x) if out is None else out
    check(lib().aha_hip_debug_layernorm_rows(_ptr(x), _ptr(w), _ptr(b), _ptr(out), x.shape[0] if rows is None else int(rows), x.shape[-1], eps,
                                             _stream()))
    return out


def debug_gemm_layernorm(A: torch.Tensor, W: torch.Tensor, norm_w: torch.Tensor, norm_b: torch.Tensor, eps: float,
                         bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act: int = _lib.ACT_NONE,
                         out: Optional[torch.Tensor] = None, norm_out: Optional[torch.Tensor] = None):
    """Test entry (aha_hip_debug_gemm_layernorm): gemm() with LayerNorm(C; norm_w, norm_b, eps) riding on the call -> (C, norm_out), both
    (M, N) bf16 (`out` / `norm_out`: pre-filled tensors to write into)."""
    _chk(A, W, norm_w, norm_b, bias, residual, out, norm_out)
    M, K = A.shape
    N = W.shape[0]
    Cm = torch.empty(M, N, dtype=torch.bfloat16, device=A.device) if out is None else out
    Y = torch.empty(M, N, dtype=torch.bfloat16, device=A.device) if norm_out is None else norm_out
    check(lib().aha_hip_debug_gemm_layernorm(_ptr(A), _ptr(W), _ptr(Cm), M, N, K, K, W.shape[1], N, _ptr(bias), _ptr(residual), act, _ptr(norm_w),
                                             _ptr(norm_b), _ptr(Y), eps, _stream()))
    return Cm, Y


def _grids(grid_thw):
    g = np.ascontiguousarray(np.asarray(grid_thw, dtype=np.uint32).reshape(-1, 3))
    return g, int((g[:, 0].astype(np.int64) * g[:, 1] * g[:, 2]).sum())


def debug_vit_pos_embed(x: torch.Tensor, table: torch.Tensor, grid_thw, G: int, merge: int = 2):
    """Test entry (aha_hip_debug_vit_pos_embed): the tower's host corner tables for grid_thw [(t, h, w), ...] and launch_pos_embed_add on x
    (N, D) bf16 IN PLACE with table (G * G, D) bf16.  -> (idx (4, N) int32, wt (4, N) f32) numpy."""
    _chk(x, table)
    g, N = _grids(grid_thw)
    idx, wt = np.empty((4, max(N, 1)), np.int32), np.empty((4, max(N, 1)), np.float32)
    check(lib().aha_hip_debug_vit_pos_embed(g.ctypes.data, g.shape[0], int(G), int(merge), _ptr(table), _ptr(x), x.shape[0], x.shape[1],
                                            idx.ctypes.data, wt.ctypes.data, _stream()))
    return idx[:, :N], wt[:, :N]


def debug_vit_rope(qkv: torch.Tensor, grid_thw, inv_freq: torch.Tensor, page_ptrs: torch.Tensor, nh: int, q_out: torch.Tensor,
                   merge: int = 2, hd: int = 72):
    """Test entry (aha_hip_debug_vit_rope): launch_vit_rope_table, then launch_vit_rope_pack onto pages of the caller, with the tower's host
    tables for grid_thw.  qkv (N, 3 * nh * 72) bf16, inv_freq (18) f32, page_ptrs (P,) int64 device page addresses, q_out (N, nh, 96) bf16
    (pre-filled by the caller).  -> (cs_tab (N, 36, 2) f32 device tensor, rowcol (N, 2), page_of (N), slot_of (N) numpy int32)."""
    _chk(qkv, inv_freq, page_ptrs, q_out)
    assert inv_freq.dtype == torch.float32 and page_ptrs.dtype == torch.int64
    g, N = _grids(grid_thw)
    tab = torch.empty(max(N, 1), 36, 2, dtype=torch.float32, device=qkv.device)
    rowcol, page_of, slot_of = np.empty((max(N, 1), 2), np.int32), np.empty(max(N, 1), np.int32), np.empty(max(N, 1), np.int32)
    check(lib().aha_hip_debug_vit_rope(_ptr(qkv), g.ctypes.data, g.shape[0], int(merge), _ptr(inv_freq), _ptr(page_ptrs), page_ptrs.numel(),
                                       qkv.shape[0], nh, hd, _ptr(tab), _ptr(q_out), rowcol.ctypes.data, page_of.ctypes.data, slot_of.ctypes.data,
                                       _stream()))
    return tab[:N], rowcol[:N], page_of[:N], slot_of[:N]


def debug_scatter_rows(dst: torch.Tensor, src: torch.Tensor, rows, add: bool) -> None:
    """Test entry (aha_hip_debug_scatter_rows): dst[rows[i]] = src[i] (or bf16(dst + src) with add), in place."""
    _chk(dst, src)
    r = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
    assert r.size == src.shape[0] and dst.shape[1] == src.shape[1]
    check(lib().aha_hip_debug_scatter_rows(_ptr(dst), _ptr(src), r.ctypes.data, r.size, dst.shape[0], dst.shape[1], int(bool(add)), _stream()))


def debug_audio_im2col1(feat: torch.Tensor, chunks, out: torch.Tensor, win: int = 100) -> torch.Tensor:
    """Test entry (aha_hip_debug_audio_im2col1): feat (mels, ld) f32, chunks [(first column, F, window), ...] -> out (C * ceil(mels / 2) *
    ceil(win / 2), 16) bf16 (pre-filled by the caller)."""
    _chk(feat, out)
    assert feat.dtype == torch.float32
    c = np.ascontiguousarray(np.asarray(chunks, dtype=np.int32).reshape(-1, 3))
    check(lib().aha_hip_debug_audio_im2col1(_ptr(feat), feat.shape[1], c.ctypes.data, c.shape[0], feat.shape[0], int(win), _ptr(out), _stream()))
    return out


def debug_im2col_nhwc(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Test entry (aha_hip_debug_im2col_nhwc): x (B, Hin, Win, Cin) bf16 -> out (B * ceil(Hin / 2) * ceil(Win / 2), 9 * Cin)."""
    _chk(x, out)
    B, Hin, Win, Cin = x.shape
    check(lib().aha_hip_debug_im2col_nhwc(_ptr(x), _ptr(out), B, Hin, Win, Cin, _stream()))
    return out


def debug_audio_tokens_gather(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Test entry (aha_hip_debug_audio_tokens_gather): x (B, Fq, T, Cc) bf16 -> out (B * T, Cc * Fq)."""
    _chk(x, out)
    B, Fq, T, Cc = x.shape
    check(lib().aha_hip_debug_audio_tokens_gather(_ptr(x), _ptr(out), B, Fq, T, Cc, _stream()))
    return out


def debug_sinus_pe_add(x: torch.Tensor, T: int, rows: Optional[int] = None) -> torch.Tensor:
    """Test entry (aha_hip_debug_sinus_pe_add): x (R, d) bf16 IN PLACE over the first `rows` rows, row r at position r % T."""
    _chk(x)
    check(lib().aha_hip_debug_sinus_pe_add(_ptr(x), x.shape[0] if rows is None else int(rows), x.shape[1], int(T), _stream()))
    return x


def debug_kv_pack_generic(src: torch.Tensor, k_off: int, v_off: int, page_ptrs: torch.Tensor, nh: int, hd: int, slot_of=None,
                          rows: Optional[int] = None) -> None:
    """Test entry (aha_hip_debug_kv_pack_generic): the K / V heads at columns k_off / v_off of src (N, ld) bf16 -> pages of the caller;
    slot_of: host ints, the cache slot of every row (None: row n in slot n)."""
    _chk(src, page_ptrs)
    assert page_ptrs.dtype == torch.int64
    N = src.shape[0] if rows is None else int(rows)
    s = None if slot_of is None else np.ascontiguousarray(np.asarray(slot_of, dtype=np.int32).reshape(N))
    check(lib().aha_hip_debug_kv_pack_generic(_ptr(src), src.shape[1], int(k_off), int(v_off), _ptr(page_ptrs), page_ptrs.numel(), N, nh, hd,
                                              None if s is None else s.ctypes.data, _stream()))


def argmax(x: torch.Tensor) -> int:
    _chk(x)
    assert x.dtype == torch.float32
    out = torch.zeros(1, dtype=torch.int32, device=x.device)
    check(lib().aha_hip_argmax(_ptr(x), x.numel(), _ptr(out), _stream()))
    return int(out.item()) & 0xFFFFFFFF


def bf16_scale(d: int) -> float:
    """1/sqrt(d) rounded to bf16: the scalar of Candle's `attn_weights * scaling` affine op is cast to the tensor dtype."""
    return float(torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32).bfloat16().float())


def image_to_patches(img_u8_hwc: torch.Tensor, patch: int = 16, merge: int = 2, mean=(0.5, 0.5, 0.5),
                     std=(0.5, 0.5, 0.5)) -> torch.Tensor:
    """V0: (H, W, 3) uint8 GPU tensor -> (N, 3*2*patch*patch) bf16 pixel_values rows (frame duplicated, merge order)."""
    import ctypes as C
    _chk(img_u8_hwc)
    assert img_u8_hwc.dtype == torch.uint8 and img_u8_hwc.dim() == 3 and img_u8_hwc.shape[2] == 3
    H, W = int(img_u8_hwc.shape[0]), int(img_u8_hwc.shape[1])
    out = torch.empty((H // patch) * (W // patch), 6 * patch * patch, dtype=torch.bfloat16, device=img_u8_hwc.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    check(lib().aha_hip_image_to_patches(_ptr(img_u8_hwc), _ptr(out), H, W, patch, merge, m, s, _stream()))
    return out


def video_to_patches(frames_u8_thwc: torch.Tensor, patch: int = 16, merge: int = 2, mean=(0.5, 0.5, 0.5),
                     std=(0.5, 0.5, 0.5)) -> torch.Tensor:
    """process_videos: (T, H, W, 3) uint8 GPU frames -> (ceil(T/2)*N, 3*2*patch*patch) bf16 rows (frame pairs, an odd last frame
    repeated; normalised in bf16 op by op like the reference's video path)."""
    import ctypes as C
    _chk(frames_u8_thwc)
    assert frames_u8_thwc.dtype == torch.uint8 and frames_u8_thwc.dim() == 4 and frames_u8_thwc.shape[3] == 3
    T, H, W = (int(x) for x in frames_u8_thwc.shape[:3])
    out = torch.empty(((T + 1) // 2) * (H // patch) * (W // patch), 6 * patch * patch, dtype=torch.bfloat16, device=frames_u8_thwc.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    check(lib().aha_hip_video_to_patches(_ptr(frames_u8_thwc), _ptr(out), T, H, W, patch, merge, m, s, _stream()))
    return out


def image_resize(img_u8_hwc: torch.Tensor, new_h: int, new_w: int) -> torch.Tensor:
    """V0-pre: DynamicImage::resize_exact(new_w, new_h, CatmullRom) of an RGB8 (H, W, 3) image on the GPU."""
    _chk(img_u8_hwc)
    assert img_u8_hwc.dtype == torch.uint8 and img_u8_hwc.dim() == 3 and img_u8_hwc.shape[2] == 3
    H, W = int(img_u8_hwc.shape[0]), int(img_u8_hwc.shape[1])
    out = torch.empty(new_h, new_w, 3, dtype=torch.uint8, device=img_u8_hwc.device)
    check(lib().aha_hip_image_resize(_ptr(img_u8_hwc), H, W, _ptr(out), new_h, new_w, _stream()))
    return out


def logmel(samples: torch.Tensor) -> torch.Tensor:
    """A0: 16 kHz mono f32 samples on the GPU -> Whisper log-mel features (128, n_samples // 160) f32."""
    _chk(samples)
    assert samples.dtype == torch.float32 and samples.dim() == 1
    out = torch.empty(128, samples.numel() // 160, dtype=torch.float32, device=samples.device)
    check(lib().aha_hip_logmel(_ptr(samples), samples.numel(), _ptr(out), _stream()))
    return out


def logmel_batch(clips) -> torch.Tensor:
    """A0 over many clips in one launch pair (aha_hip_logmel_batch): a list of 1-D f32 sample tensors on one GPU -> (128, sum F_j) f32,
    F_j = len(clip j) // 160, clip j's frames in its own columns (bit-identical to logmel(clip j))."""
    assert len(clips) > 0
    for c in clips:
        _chk(c)
        assert c.dtype == torch.float32 and c.dim() == 1
    flat = torch.cat([c.reshape(-1) for c in clips]).contiguous()
    n = np.ascontiguousarray([c.numel() for c in clips], dtype=np.int64)
    out = torch.empty(128, int((n // 160).sum()), dtype=torch.float32, device=flat.device)
    check(lib().aha_hip_logmel_batch(_ptr(flat), n.ctypes.data, len(clips), _ptr(out), _stream()))
    return out


# ---- batched decode (aha_hip_generate_batch's kernels) ----------------------------------------------------------------------
GEMV_ROWS_STORE, GEMV_ROWS_RESIDUAL, GEMV_ROWS_SILU_MUL, GEMV_ROWS_LOGITS = 0, 1, 2, 3


def _gemv_rows_outputs(R: int, N: int, epi: int, device, out: Optional[torch.Tensor]):
    """(y, logits, argmax) of a gemv_rows call.  `out`: the caller's (R, N_out) bf16 tensor for the bf16 epilogues -- rows of a larger
    buffer, or the residual itself (the in-place form the model runs)."""
    y = logits = am = None
    if epi == GEMV_ROWS_LOGITS:
        if out is not None:
            raise ValueError("gemv_rows: out= is for the bf16 epilogues")
        logits = torch.empty(R, N, dtype=torch.float32, device=device)
        am = torch.empty(R, dtype=torch.int32, device=device)
    else:
        shape = (R, N // 2 if epi == GEMV_ROWS_SILU_MUL else N)
        if out is not None and (out.dtype != torch.bfloat16 or tuple(out.shape) != shape):
            raise ValueError(f"gemv_rows: out must be {shape} bf16")
        y = out if out is not None else torch.empty(shape, dtype=torch.bfloat16, device=device)
    return y, logits, am


def gemv_rows(W: torch.Tensor, x: torch.Tensor, epi: int = GEMV_ROWS_STORE, residual: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None):
    """y[R, N] = x[R, K] . W[N, K]^T for 1 <= R <= 32, weights streamed once.  epi STORE / RESIDUAL -> (R, N) bf16 (`out` may be the
    residual itself); SILU_MUL (W in the 16-row gate / up block layout) -> (R, N/2) bf16; LOGITS -> ((R, N) f32 logits, (R,) int64 argmax)."""
    _chk(W, x, residual, out)
    N, K = W.shape
    R = x.shape[0]
    y, logits, am = _gemv_rows_outputs(R, N, epi, x.device, out)
    check(lib().aha_hip_gemv_rows(_ptr(W), _ptr(x), _ptr(y), R, N, K, epi, _ptr(residual), _ptr(logits), _ptr(am), _stream()))
    return (logits, am.long()) if epi == GEMV_ROWS_LOGITS else y


def _quantize_mx(entry, W: torch.Tensor, k_per_byte: int):
    """One of the library's MX quantisers on a GPU bf16 matrix (N, K): q holds k_per_byte elements per byte."""
    from . import quant
    _chk(W)
    N, K = W.shape
    q = torch.empty(N, K // k_per_byte, dtype=torch.uint8, device=W.device)
    words = torch.empty(N, (K + 127) // 128, dtype=torch.int32, device=W.device)
    wr = torch.empty_like(W)
    check(entry(_ptr(W), N, K, _ptr(q), _ptr(words), _ptr(wr), _stream()))
    return q, quant.scales_from_kernel(words, K).to(W.device), wr


def _gemv_rows_mx(entry, q: torch.Tensor, K: int, scales: torch.Tensor, x: torch.Tensor, epi: int, residual: Optional[torch.Tensor],
                  out: Optional[torch.Tensor] = None):
    """gemv_rows from an MX copy (q, scales) of a matrix with K columns, through the C entry of its format."""
    from . import quant
    _chk(q, x, residual, out)
    N, R = q.shape[0], x.shape[0]
    words = quant.scales_to_kernel(scales).to(x.device)
    y, logits, am = _gemv_rows_outputs(R, N, epi, x.device, out)
    check(entry(_ptr(q), _ptr(words), _ptr(x), _ptr(y), R, N, K, epi, _ptr(residual), _ptr(logits), _ptr(am), _stream()))
    return (logits, am.long()) if epi == GEMV_ROWS_LOGITS else y


def quantize_mxfp8(W: torch.Tensor):
    """The library's MXFP8 quantiser (aha_hip_quantize_mxfp8) on a GPU bf16 matrix (N, K), K % 32 == 0 -> (q (N, K) uint8, scales
    (N, K / 32) uint8, W' (N, K) bf16) on the GPU, scales in the reference's order (aha_amd/quant.py quantize_mxfp8: the same bytes)."""
    return _quantize_mx(lib().aha_hip_quantize_mxfp8, W, 1)


def gemv_rows_mxfp8(q: torch.Tensor, scales: torch.Tensor, x: torch.Tensor, epi: int = GEMV_ROWS_STORE, residual: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None):
    """gemv_rows from the MXFP8 copy of W: q (N, K) uint8, scales (N, K / 32) uint8 in the reference's order (converted to the kernel's
    words here).  Every output bit equals gemv_rows(W', x, epi, residual) for W' = dequantize_mxfp8(q, scales)."""
    return _gemv_rows_mx(lib().aha_hip_gemv_rows_mxfp8, q, q.shape[1], scales, x, epi, residual, out)


def quantize_mxfp4(W: torch.Tensor):
    """The library's MXFP4 quantiser (aha_hip_quantize_mxfp4) on a GPU bf16 matrix (N, K), K % 32 == 0 -> (q (N, K / 2) uint8 packed E2M1
    codes, scales (N, K / 32) uint8, W' (N, K) bf16) on the GPU, scales in the reference's order (aha_amd/quant.py quantize_mxfp4: the same
    bytes)."""
    return _quantize_mx(lib().aha_hip_quantize_mxfp4, W, 2)


def gemv_rows_mxfp4(q: torch.Tensor, scales: torch.Tensor, x: torch.Tensor, epi: int = GEMV_ROWS_STORE, residual: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None):
    """gemv_rows from the MXFP4 copy of W: q (N, K / 2) uint8 packed E2M1 codes, scales (N, K / 32) uint8 in the reference's order
    (converted to the kernel's words here).  Every output bit equals gemv_rows(W', x, epi, residual) for W' = dequantize_mxfp4(q, scales)."""
    _chk(q, x, residual, out)
    N, K = q.shape[0], q.shape[1] * 2
    if scales.shape != (N, K // 32) or x.shape[1] != K:
        raise ValueError(f"gemv_rows_mxfp4: q {tuple(q.shape)} wants scales ({N}, {K // 32}) and x (R, {K})")
    return _gemv_rows_mx(lib().aha_hip_gemv_rows_mxfp4, q, K, scales, x, epi, residual, out)


def _gemv_epi_outputs(N: int, epi: int, device, out: Optional[torch.Tensor]):
    y = logits = am = None
    if epi == GEMV_ROWS_LOGITS:
        logits = torch.empty(N, dtype=torch.float32, device=device)
        am = torch.empty(1, dtype=torch.int32, device=device)
    else:
        y = out if out is not None else torch.empty(N // 2 if epi == GEMV_ROWS_SILU_MUL else N, dtype=torch.bfloat16, device=device)
    return y, logits, am


def gemv_epi(W: torch.Tensor, x: torch.Tensor, epi: int = GEMV_ROWS_STORE, norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6,
             residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """The single-sequence decode matvec with an epilogue (aha_hip_gemv_epi): W (N, K) bf16, x (K) bf16, epi as in gemv_rows -- STORE /
    RESIDUAL -> (N) bf16 (`out` may be the residual itself); SILU_MUL (W in the 16-row gate / up block layout) -> (N / 2) bf16; LOGITS ->
    ((N) f32 logits, int argmax).  norm_w fuses RMSNorm(x; norm_w, eps) in front."""
    _chk(W, x, norm_w, residual, out)
    N, K = W.shape
    y, logits, am = _gemv_epi_outputs(N, epi, x.device, out)
    check(lib().aha_hip_gemv_epi(_ptr(W), _ptr(x), _ptr(y), N, K, epi, _ptr(norm_w), eps, _ptr(residual), _ptr(logits), _ptr(am), _stream()))
    return (logits, int(am.item())) if epi == GEMV_ROWS_LOGITS else y


def plan_gemv(N: int, K: int, epi: int = GEMV_ROWS_STORE, has_norm: bool = False):
    """Host only: (R, U, grid, form) the bf16 matvec picks for a matrix of N rows (epi 2: N = 2I, either weight layout; epi 4: the f32
    partial sums) (aha_hip_debug_plan_gemv): form 0 general, 1 FAST, 2 / 3 FAST with the straight-line prologue without / with norm weights."""
    r, u, g, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().aha_hip_debug_plan_gemv(N, K, epi, int(has_norm), C.byref(r), C.byref(u), C.byref(g), C.byref(f)))
    return r.value, u.value, g.value, f.value


def plan_gemv_rows(N: int, K: int):
    """Host only: (cw, nks) of gemv_rows and its MX twins for a matrix of N rows and K columns (aha_hip_debug_plan_gemv_rows): chunks per
    wave and K splits; with the row tiles (2 above 16 rows) the launch is gemv_rows_kernel<cw, 1 | 2>."""
    cw, nks = C.c_int32(), C.c_int32()
    check(lib().aha_hip_debug_plan_gemv_rows(N, K, C.byref(cw), C.byref(nks)))
    return cw.value, nks.value


def gemv_partial_f32(W: torch.Tensor, x: torch.Tensor, norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """Test entry (aha_hip_debug_gemv_partial_f32): the bf16 matvec's un-rounded f32 sums, the epilogue of a sharded model's row-parallel
    projections.  W (N, K) bf16, x (K) bf16 -> (N) f32."""
    _chk(W, x, norm_w)
    N, K = W.shape
    y = torch.empty(N, dtype=torch.float32, device=x.device)
    check(lib().aha_hip_debug_gemv_partial_f32(_ptr(W), _ptr(x), _ptr(y), N, K, _ptr(norm_w), eps, _stream()))
    return y


def gemv_mxfp8(q: torch.Tensor, scales: torch.Tensor, x: torch.Tensor, epi: int = GEMV_ROWS_STORE, norm_w: Optional[torch.Tensor] = None,
               eps: float = 1e-6, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """gemv_epi from the MXFP8 copy of W (aha_hip_gemv_mxfp8): q (N, K) uint8, scales (N, K / 32) uint8 in the reference's order (converted
    to the kernel's words here).  Every output bit, and the argmax, equals gemv_epi(W', ...) for W' = dequantize_mxfp8(q, scales)."""
    from . import quant
    _chk(q, x, norm_w, residual, out)
    N, K = q.shape
    words = quant.scales_to_kernel(scales).to(x.device)
    y, logits, am = _gemv_epi_outputs(N, epi, x.device, out)
    check(lib().aha_hip_gemv_mxfp8(_ptr(q), _ptr(words), _ptr(x), _ptr(y), N, K, epi, _ptr(norm_w), eps, _ptr(residual), _ptr(logits), _ptr(am),
                                   _stream()))
    return (logits, int(am.item())) if epi == GEMV_ROWS_LOGITS else y


def plan_gemv_mxfp8(N: int, K: int, epi: int = GEMV_ROWS_STORE, has_norm: bool = False):
    """Host only: (R, U, grid, form) gemv_mxfp8 picks for a matrix of N rows (aha_hip_debug_plan_gemv_mxfp8): form 0 general, 1 FAST, 2 / 3
    FAST with the straight-line prologue without / with norm weights."""
    r, u, g, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().aha_hip_debug_plan_gemv_mxfp8(N, K, epi, int(has_norm), C.byref(r), C.byref(u), C.byref(g), C.byref(f), None))
    return r.value, u.value, g.value, f.value


def gemv_mxfp8_by_plan(N: int, K: int, epi: int = GEMV_ROWS_STORE) -> bool:
    """Host only: does a quantised model's single-sequence step read a matrix of N rows (gate+up: 2I) and K columns from its copy?"""
    r, b = C.c_int32(), C.c_int32()
    check(lib().aha_hip_debug_plan_gemv_mxfp8(N, K, epi, 0, C.byref(r), C.byref(r), C.byref(r), None, C.byref(b)))
    return bool(b.value)


def pack_pk13(W: torch.Tensor, check_only: bool = False):
    """The exact 13-bit copy of a bf16 matrix W (N, K) on the GPU, K % 4096 == 0 (aha_hip_pack_pk13; quant.pack_pk13 is its restatement):
    (packed (N, K / 4096, 6656) uint8 or None, bh, bad).  bad != 0: W holds that many weights the format cannot keep, and nothing is packed."""
    _chk(W)
    N, K = W.shape
    bh, bad = C.c_int32(), C.c_int64()
    out = None if check_only else torch.zeros(N, K // 4096, 6656, dtype=torch.uint8, device=W.device)
    check(lib().aha_hip_pack_pk13(_ptr(W), N, K, _ptr(out), C.byref(bh), C.byref(bad), _stream()))
    return (out if bad.value == 0 else None), bh.value, bad.value


def gemv_pk13(packed: torch.Tensor, bh: int, x: torch.Tensor, epi: int = GEMV_ROWS_STORE, norm_w: Optional[torch.Tensor] = None,
              eps: float = 1e-6, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """gemv_epi from the exact 13-bit copy of W (aha_hip_gemv_pk13): packed (N, K / 4096, 6656) uint8 and its base bh.  Every output bit,
    and the argmax, equals gemv_epi(W, ...)."""
    _chk(packed, x, norm_w, residual, out)
    N, K = packed.shape[0], packed.shape[1] * 4096
    y, logits, am = _gemv_epi_outputs(N, epi, x.device, out)
    check(lib().aha_hip_gemv_pk13(_ptr(packed), bh, _ptr(x), _ptr(y), N, K, epi, _ptr(norm_w), eps, _ptr(residual), _ptr(logits), _ptr(am),
                                  _stream()))
    return (logits, int(am.item())) if epi == GEMV_ROWS_LOGITS else y


def pack_pk13_rows(W: torch.Tensor, cap: int = 16, check_only: bool = False):
    """pack_pk13 for a matrix that may hold finite weights below the window (aha_hip_pack_pk13_rows; quant.check_pk13_rows / pack_pk13_rows
    are its restatement): (packed or None, bh, rows, below, nonfinite).  rows: the rows of W (ascending, at most 16) that hold such a weight
    and that gemv_pk13_rows reads from W itself, or None if there are more than 16.  Packed if nonfinite == 0 and len(rows) <= cap."""
    _chk(W)
    N, K = W.shape
    bh, n, below, nonfinite = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    rows = (C.c_int32 * 16)()
    out = None if check_only else torch.zeros(N, K // 4096, 6656, dtype=torch.uint8, device=W.device)
    check(lib().aha_hip_pack_pk13_rows(_ptr(W), N, K, _ptr(out), C.byref(bh), rows, cap, C.byref(n), C.byref(below), C.byref(nonfinite), _stream()))
    got = None if n.value > 16 else [int(rows[i]) for i in range(min(n.value, cap))]
    ok = nonfinite.value == 0 and n.value <= cap
    return (out if ok else None), bh.value, got, below.value, nonfinite.value


def gemv_pk13_rows(packed: torch.Tensor, bh: int, W: Optional[torch.Tensor], rows, x: torch.Tensor, epi: int = GEMV_ROWS_STORE,
                   norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6, residual: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None):
    """gemv_pk13 with exception rows (aha_hip_gemv_pk13_rows): the rows of W listed in `rows` (at most 16) are computed from the bf16 matrix
    W, every other row from the copy.  Every output bit, and the argmax, equals gemv_epi(W, ...).  An empty list is gemv_pk13."""
    _chk(packed, x, norm_w, residual, out)
    if W is not None:
        _chk(W)
    N, K = packed.shape[0], packed.shape[1] * 4096
    rows = [int(r) for r in rows]
    arr = (C.c_int32 * max(len(rows), 1))(*rows)
    y, logits, am = _gemv_epi_outputs(N, epi, x.device, out)
    check(lib().aha_hip_gemv_pk13_rows(_ptr(packed), bh, _ptr(W), arr, len(rows), _ptr(x), _ptr(y), N, K, epi, _ptr(norm_w), eps, _ptr(residual),
                                       _ptr(logits), _ptr(am), _stream()))
    return (logits, int(am.item())) if epi == GEMV_ROWS_LOGITS else y


def plan_gemv_pk13(N: int, K: int, epi: int = GEMV_ROWS_STORE, has_norm: bool = False):
    """Host only: (R, U, grid, form) gemv_pk13 picks for a matrix of N rows (aha_hip_debug_plan_gemv_pk13): U is 8, form 1 FAST, 2 / 3 FAST
    with the straight-line prologue without / with norm weights."""
    r, u, g, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().aha_hip_debug_plan_gemv_pk13(N, K, epi, int(has_norm), C.byref(r), C.byref(u), C.byref(g), C.byref(f), None))
    return r.value, u.value, g.value, f.value


def gemv_pk13_by_plan(N: int, K: int, epi: int = GEMV_ROWS_STORE) -> bool:
    """Host only: does a model's single-sequence step read a matrix of N rows (gate+up: 2I) and K columns from its exact 13-bit copy?"""
    if N < 1 or K < 4096 or K % 4096 or K > 32768:      # not a shape of the kernel at all
        return False
    r, b = C.c_int32(), C.c_int32()
    check(lib().aha_hip_debug_plan_gemv_pk13(N, K, epi, 0, C.byref(r), C.byref(r), C.byref(r), None, C.byref(b)))
    return bool(b.value)


def gemv_mxfp4(q: torch.Tensor, scales: torch.Tensor, x: torch.Tensor, epi: int = GEMV_ROWS_STORE, norm_w: Optional[torch.Tensor] = None,
               eps: float = 1e-6, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """gemv_epi from the MXFP4 copy of W (aha_hip_gemv_mxfp4): q (N, K / 2) uint8 packed E2M1 codes, scales (N, K / 32) uint8 in the
    reference's order (converted to the kernel's words here).  Every output bit, and the argmax, equals gemv_epi(W', ...) for W' =
    dequantize_mxfp4(q, scales)."""
    from . import quant
    _chk(q, x, norm_w, residual, out)
    N, K = q.shape[0], q.shape[1] * 2
    if scales.shape != (N, K // 32) or x.shape[0] != K:
        raise ValueError(f"gemv_mxfp4: q {tuple(q.shape)} wants scales ({N}, {K // 32}) and x ({K})")
    words = quant.scales_to_kernel(scales).to(x.device)
    y, logits, am = _gemv_epi_outputs(N, epi, x.device, out)
    check(lib().aha_hip_gemv_mxfp4(_ptr(q), _ptr(words), _ptr(x), _ptr(y), N, K, epi, _ptr(norm_w), eps, _ptr(residual), _ptr(logits), _ptr(am),
                                   _stream()))
    return (logits, int(am.item())) if epi == GEMV_ROWS_LOGITS else y


def plan_gemv_mxfp4(N: int, K: int, epi: int = GEMV_ROWS_STORE, has_norm: bool = False):
    """Host only: (R, U, grid, form) gemv_mxfp4 picks for a matrix of N rows (aha_hip_debug_plan_gemv_mxfp4), form as plan_gemv_mxfp8's."""
    r, u, g, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().aha_hip_debug_plan_gemv_mxfp4(N, K, epi, int(has_norm), C.byref(r), C.byref(u), C.byref(g), C.byref(f), None))
    return r.value, u.value, g.value, f.value


def gemv_mxfp4_by_plan(N: int, K: int, epi: int = GEMV_ROWS_STORE) -> bool:
    """Host only: does an MXFP4 model's single-sequence step read a matrix of N rows (gate+up: 2I) and K columns from its copy?"""
    r, b = C.c_int32(), C.c_int32()
    check(lib().aha_hip_debug_plan_gemv_mxfp4(N, K, epi, 0, C.byref(r), C.byref(r), C.byref(r), None, C.byref(b)))
    return bool(b.value)


def attn_decode_batch(qkv: torch.Tensor, q_norm_w: torch.Tensor, k_norm_w: torch.Tensor, rope: torch.Tensor, page_ptrs: torch.Tensor,
                      page0, kv_len, nh: int, kvh: int, eps: float, scale: float) -> torch.Tensor:
    """Fused decode attention of R sequences in one launch: qkv (R, (nh+2kvh)*128) bf16, rope (R, 128) f32, page_ptrs (P,) int64 device
    page addresses, page0 / kv_len: per-row first page and cache length after the append (host ints).  -> (R, nh*128) bf16."""
    _chk(qkv, q_norm_w, k_norm_w, rope, page_ptrs)
    R = qkv.shape[0]
    p0 = np.ascontiguousarray(np.asarray(page0, dtype=np.int32))
    kl = np.ascontiguousarray(np.asarray(kv_len, dtype=np.int32))
    o = torch.empty(R, nh * 128, dtype=torch.bfloat16, device=qkv.device)
    check(lib().aha_hip_attn_decode_batch(_ptr(qkv), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(rope), _ptr(page_ptrs), p0.ctypes.data,
                                          kl.ctypes.data, R, nh, kvh, eps, scale, _ptr(o), _stream()))
    return o


def debug_attn_decode_fused(qkv_row: torch.Tensor, q_norm_w: torch.Tensor, k_norm_w: torch.Tensor, rope_row: torch.Tensor,
                            page_ptrs: torch.Tensor, kv_len: int, nh: int, kvh: int, eps: float, scale: float) -> torch.Tensor:
    """The single-sequence fused decode attention kernel on one sequence whose pages are page_ptrs[0 ..]: -> (nh*128) bf16."""
    _chk(qkv_row, q_norm_w, k_norm_w, rope_row, page_ptrs)
    o = torch.empty(nh * 128, dtype=torch.bfloat16, device=qkv_row.device)
    check(lib().aha_hip_debug_attn_decode_fused(_ptr(qkv_row), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(rope_row), _ptr(page_ptrs), int(kv_len),
                                                nh, kvh, eps, scale, _ptr(o), _stream()))
    return o


ATTN_ROWS_FUSED, ATTN_ROWS_APPEND_THEN_ATTEND, ATTN_ROWS_APPEND_ONLY = 0, 1, 2
SPEC_MAX_DRAFT, SPEC_OUT_WORDS = 15, 18   # kernels.h: the accept record is {count, last row, tokens[16]}


def debug_attn_decode_rows(qkv: torch.Tensor, q_norm_w: torch.Tensor, k_norm_w: torch.Tensor, rope: torch.Tensor, page_ptrs: torch.Tensor,
                           page0, kv_len, nh: int, kvh: int, eps: float, scale: float, form: int) -> Optional[torch.Tensor]:
    """Test entry (aha_hip_debug_attn_decode_rows): attn_decode_batch's arguments, rows of one sequence allowed (the same page0, kv_len
    ascending by one: a last token and its drafts).  form 0: the default launch (append inside the attention); 1: the KV append of every
    row, then the attention without its append, as a draft-and-verify step queues them; 2: the append alone.  -> (R, nh*128) bf16, None
    for form 2."""
    _chk(qkv, q_norm_w, k_norm_w, rope, page_ptrs)
    R = qkv.shape[0]
    p0 = np.ascontiguousarray(np.asarray(page0, dtype=np.int32).reshape(R))
    kl = np.ascontiguousarray(np.asarray(kv_len, dtype=np.int32).reshape(R))
    o = None if form == ATTN_ROWS_APPEND_ONLY else torch.empty(R, nh * 128, dtype=torch.bfloat16, device=qkv.device)
    check(lib().aha_hip_debug_attn_decode_rows(_ptr(qkv), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(rope), _ptr(page_ptrs), p0.ctypes.data,
                                               kl.ctypes.data, R, nh, kvh, eps, scale, _ptr(o), int(form), _stream()))
    return o


def debug_spec_accept(argmax: torch.Tensor, row_tok, seq_tab, layout: int) -> torch.Tensor:
    """Test entry (aha_hip_debug_spec_accept): the accept kernel of a draft-and-verify step.  argmax (rows) int32 / uint32 on the device,
    row_tok: the rows' input tokens (host ints), seq_tab: per sequence (row0, n_draft) for layout 0 (spec_accept_rows_kernel) or (own row,
    first draft row, n_draft) for layout 1 (spec_accept_split_kernel).  -> (n_seqs, 18) int32 on the device: {count, last row, tokens[16]}
    per sequence, words behind the count as allocated (0xffffffff)."""
    _chk(argmax)
    assert argmax.dim() == 1 and argmax.element_size() == 4
    rows = argmax.numel()
    tok = np.ascontiguousarray(np.asarray(row_tok, dtype=np.int64).reshape(rows).astype(np.int32))
    seq = np.ascontiguousarray(np.asarray(seq_tab, dtype=np.int32).reshape(-1, 3 if layout else 2))
    out = torch.full((seq.shape[0], SPEC_OUT_WORDS), -1, dtype=torch.int32, device=argmax.device)
    check(lib().aha_hip_debug_spec_accept(_ptr(argmax), tok.ctypes.data, rows, seq.ctypes.data, seq.shape[0], int(layout), _ptr(out), _stream()))
    return out


def sample_rows(logits: torch.Tensor, k, temperature, repeat_penalty, contexts):
    """aha_hip_sample_candidates for every row of logits (R, V) f32 (row pitch logits.stride(0)) in one launch per stage: row r with
    k[r] (1..64), temperature[r], repeat_penalty[r] over the ids contexts[r].  The logits are only read.  -> (vals (R, 64) f32,
    idx (R, 64) int32, ms (R, 2) f32 = {max, sumexp}); the first k[r] entries of row r are its candidates."""
    _chk(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    R, V = logits.shape
    kk = np.ascontiguousarray(np.asarray(k, dtype=np.int32).reshape(R))
    tt = np.ascontiguousarray(np.asarray(temperature, dtype=np.float32).reshape(R))
    pp = np.ascontiguousarray(np.asarray(repeat_penalty, dtype=np.float32).reshape(R))
    off = np.ascontiguousarray(np.cumsum([0] + [len(c) for c in contexts]), dtype=np.uint64)
    ctx = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32).reshape(-1) for c in contexts] + [np.zeros(1, np.uint32)]))
    vals = torch.empty(R, 64, dtype=torch.float32, device=logits.device)
    idx = torch.empty(R, 64, dtype=torch.int32, device=logits.device)
    ms = torch.empty(R, 2, dtype=torch.float32, device=logits.device)
    check(lib().aha_hip_sample_rows(_ptr(logits), logits.stride(0), R, V, kk.ctypes.data, tt.ctypes.data, pp.ctypes.data, ctx.ctypes.data,
                                    off.ctypes.data, _ptr(vals), _ptr(idx), _ptr(ms), _stream()))
    return vals, idx, ms


def sample_rows_adjusted(logits: torch.Tensor, k, temperature, repeat_penalty, contexts, adjusts):
    """sample_rows with addends (aha_hip_sample_rows_adjusted): adjusts[r] = (ids, vals) -- vals[i] (finite or -inf) is added, in f32, to the
    penalised logit of the distinct ids[i] < V of row r, in any order; an empty pair gives the row sample_rows gives it.  The rows may
    have a pitch above V."""
    if not logits.is_cuda:
        raise ValueError("op inputs must be GPU tensors")
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]   # (a row pitch)
    R, V = logits.shape
    assert len(adjusts) == R
    kk = np.ascontiguousarray(np.asarray(k, dtype=np.int32).reshape(R))
    tt = np.ascontiguousarray(np.asarray(temperature, dtype=np.float32).reshape(R))
    pp = np.ascontiguousarray(np.asarray(repeat_penalty, dtype=np.float32).reshape(R))
    off = np.ascontiguousarray(np.cumsum([0] + [len(c) for c in contexts]), dtype=np.uint64)
    ctx = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32).reshape(-1) for c in contexts] + [np.zeros(1, np.uint32)]))
    aoff = np.ascontiguousarray(np.cumsum([0] + [len(a[0]) for a in adjusts]), dtype=np.uint64)
    aid = np.ascontiguousarray(np.concatenate([np.asarray(a[0], dtype=np.uint32).reshape(-1) for a in adjusts] + [np.zeros(1, np.uint32)]))
    aval = np.ascontiguousarray(np.concatenate([np.asarray(a[1], dtype=np.float32).reshape(-1) for a in adjusts] + [np.zeros(1, np.float32)]))
    vals = torch.empty(R, 64, dtype=torch.float32, device=logits.device)
    idx = torch.empty(R, 64, dtype=torch.int32, device=logits.device)
    ms = torch.empty(R, 2, dtype=torch.float32, device=logits.device)
    check(lib().aha_hip_sample_rows_adjusted(_ptr(logits), logits.stride(0), R, V, kk.ctypes.data, tt.ctypes.data, pp.ctypes.data,
                                             ctx.ctypes.data, off.ctypes.data, aid.ctypes.data, aval.ctypes.data, aoff.ctypes.data, _ptr(vals),
                                             _ptr(idx), _ptr(ms), _stream()))
    return vals, idx, ms


def logprob_rows(logits: torch.Tensor, tokens, n_top):
    """aha_hip_logprob_rows: the per-token log-probability pass over every row of logits (R, V) f32 (row pitch logits.stride(0)): row r's
    emitted token tokens[r] and its n_top[r] (0..20; an int: the same for every row) most likely tokens.  The logits are only read.
    -> numpy (logprob (R,) f32, n_top (R,) int32, top_ids (R, 20) uint32, top_logprobs (R, 20) f32): one aha_token_logprobs per row."""
    if not logits.is_cuda:
        raise ValueError("op inputs must be GPU tensors")
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]   # (a row pitch)
    R, V = logits.shape
    nn = np.ascontiguousarray(np.broadcast_to(np.asarray(n_top, dtype=np.int32), (R,)))
    tok = torch.as_tensor(np.asarray(tokens, dtype=np.int64).reshape(R), dtype=torch.int64).to(torch.int32).to(logits.device)
    out = torch.empty(R, 42, dtype=torch.int32, device=logits.device)
    check(lib().aha_hip_logprob_rows(_ptr(logits), logits.stride(0), R, V, _ptr(tok), nn.ctypes.data, _ptr(out), _stream()))
    o = out.cpu().numpy()
    return (o[:, 0].copy().view(np.float32), o[:, 1].copy(), o[:, 2:22].copy().view(np.uint32), o[:, 22:42].copy().view(np.float32))


def sample_rows_masked(logits: torch.Tensor, k, temperature, repeat_penalty, contexts, adjusts, masks: torch.Tensor, mask_rows):
    """sample_rows_adjusted with allowed-token masks (aha_hip_sample_rows_masked): masks (n_masks, ceil(V / 32)) int32 / uint32 words on the
    device -- id i of a mask is allowed iff bit i & 31 of word i >> 5 is set, bits at positions >= V are ignored -- and mask_rows[r] the
    mask of row r, or -1 for none.  Every logit that is not allowed becomes -inf after the penalty and the addends.  adjusts None: no addends."""
    if not logits.is_cuda or not masks.is_cuda:
        raise ValueError("op inputs must be GPU tensors")
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]   # (a row pitch)
    R, V = logits.shape
    W = (V + 31) // 32
    assert masks.dim() == 2 and masks.shape[1] == W and masks.is_contiguous() and masks.element_size() == 4
    mr = np.ascontiguousarray(np.asarray(mask_rows, dtype=np.int32).reshape(R))
    assert ((mr >= -1) & (mr < masks.shape[0])).all(), "mask_rows name masks that do not exist"
    adjusts = [([], [])] * R if adjusts is None else adjusts
    assert len(adjusts) == R
    kk = np.ascontiguousarray(np.asarray(k, dtype=np.int32).reshape(R))
    tt = np.ascontiguousarray(np.asarray(temperature, dtype=np.float32).reshape(R))
    pp = np.ascontiguousarray(np.asarray(repeat_penalty, dtype=np.float32).reshape(R))
    off = np.ascontiguousarray(np.cumsum([0] + [len(c) for c in contexts]), dtype=np.uint64)
    ctx = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32).reshape(-1) for c in contexts] + [np.zeros(1, np.uint32)]))
    aoff = np.ascontiguousarray(np.cumsum([0] + [len(a[0]) for a in adjusts]), dtype=np.uint64)
    aid = np.ascontiguousarray(np.concatenate([np.asarray(a[0], dtype=np.uint32).reshape(-1) for a in adjusts] + [np.zeros(1, np.uint32)]))
    aval = np.ascontiguousarray(np.concatenate([np.asarray(a[1], dtype=np.float32).reshape(-1) for a in adjusts] + [np.zeros(1, np.float32)]))
    vals = torch.empty(R, 64, dtype=torch.float32, device=logits.device)
    idx = torch.empty(R, 64, dtype=torch.int32, device=logits.device)
    ms = torch.empty(R, 2, dtype=torch.float32, device=logits.device)
    check(lib().aha_hip_sample_rows_masked(_ptr(logits), logits.stride(0), R, V, kk.ctypes.data, tt.ctypes.data, pp.ctypes.data, ctx.ctypes.data,
                                           off.ctypes.data, aid.ctypes.data, aval.ctypes.data, aoff.ctypes.data, _ptr(masks), mr.ctypes.data,
                                           _ptr(vals), _ptr(idx), _ptr(ms), _stream()))
    return vals, idx, ms
