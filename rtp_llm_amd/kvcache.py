"""Paged KV-cache layout helpers (host side, torch ops, device-agnostic).

The allocator contract is the reference's: a per-layer tensor
``[blocks, 2, nkv, page, hd]`` (bindings/OpDefs.h:24-28,201-202), K block = index 0,
V block = index 1 of dim 1 (pool index 2b / 2b+1, kv_cache_kernels.cu:58-61), plus an
fp32 scale plane ``[blocks, 2, nkv, page]`` for 8-bit caches (MHAKVCacheSpec.h:52-54).
The layout INSIDE a block is a property of the cache (``layout``, the values of ``mi355_kv_layer_t.layout``).  We own a writer
and a reader for each of them, but in the reference's engine we are not the only ones who touch the pool: its prefill op writes
the prompt, its KVCacheManager hands blocks between requests (block reuse, prefix caching).  A cache both sides touch has to be in
the reference's layout, with the V form of the decode back-end being replaced:

    KV_LAYOUT_NATIVE    K block: [nkv][page][hd]        V block: [nkv][hd][page]          (the default: MI355-native)
    KV_LAYOUT_REF       K block: [nkv][hd/x][page][x]   V block: [nkv][hd][page]          (reference, NonAsm / V1 decode back-end)
    KV_LAYOUT_REF_VVEC  K block: as REF                 V block: [nkv][page/x][hd][x]     (reference, Asm decode back-end)

with x = 16 / element bytes = 8 (kv_cache_utils.h:209-243; 16-bit caches only).  ``write_tokens`` / ``read_tokens`` are the codec
between the natural ``[T, nkv, hd]`` order and a cache in any of the three, ``convert_layout`` re-lays a whole cache (how a cache
prefilled under one layout is adopted under another).

8-bit caches (native layout only) hold the codes offset-binary (code + 128, i.e. the int8 with its top bit flipped): the attention
kernel widens bytes by placing them under an fp16 exponent, which wants unsigned bytes.  write_tokens / read_tokens take and return
the signed codes.

The hot-path writers are the HIP kernels behind ``ops.rope_kv_write*`` / ``ops.qkv_rope_kv_write*``; the functions here are the
slow-path equivalents used to import a cache somebody else filled and by the tests to read the cache back.
"""
from typing import Optional, Tuple

import torch


def alloc_layer_cache(num_blocks: int, nkv: int, page: int, hd: int, int8: bool, device,
                      dtype: torch.dtype = torch.float16) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """dtype: element type of a 16-bit cache (fp16 or bf16 -- the activation dtype of the model); ignored for INT8."""
    dt = torch.int8 if int8 else dtype
    kv = torch.zeros(num_blocks, 2, nkv, page, hd, dtype=dt, device=device)
    sc = torch.ones(num_blocks, 2, nkv, page, dtype=torch.float32, device=device) if int8 else None
    return kv, sc


def _flip(x: torch.Tensor) -> torch.Tensor:
    """signed code <-> stored byte (top bit flipped)."""
    return torch.bitwise_xor(x, torch.tensor(-128, dtype=torch.int8, device=x.device))


KV_LAYOUT_NATIVE, KV_LAYOUT_REF, KV_LAYOUT_REF_VVEC = 0, 1, 2   # = _C.KV_LAYOUT_* (this module does not need the library)
_X = 8   # elements per 16-byte vector of a 16-bit cache


def _views(kv_base: torch.Tensor):
    """the halves of a NATIVE cache as k [nb, nkv, page, hd], v [nb, nkv, hd, page]"""
    nb, _, nkv, page, hd = kv_base.shape
    flat = kv_base.view(nb, 2, nkv, page * hd)
    return flat[:, 0].unflatten(-1, (page, hd)), flat[:, 1].unflatten(-1, (hd, page))


def _natural_views(kv_base: torch.Tensor, layout: int = KV_LAYOUT_NATIVE):
    """Views of the K and V halves in NATURAL order whatever the layout: k [nb, nkv, page, hd/8, 8] (channel d = 8 * dim 3 + dim 4),
    v [nb, nkv, page/8, 8, hd] (token t = 8 * dim 2 + dim 3).  Writes through them land where the layout puts the element."""
    nb, _, nkv, page, hd = kv_base.shape
    if layout not in (KV_LAYOUT_NATIVE, KV_LAYOUT_REF, KV_LAYOUT_REF_VVEC):
        raise ValueError(f"unknown kv layout {layout}")
    if layout != KV_LAYOUT_NATIVE and kv_base.element_size() != 2:
        raise ValueError("the reference kv layouts exist for 16-bit caches only")
    if page % _X or hd % _X:
        raise ValueError(f"page={page} and hd={hd} must be multiples of {_X}")
    flat = kv_base.view(nb, 2, nkv, page * hd)
    kf, vf = flat[:, 0], flat[:, 1]
    if layout == KV_LAYOUT_NATIVE:
        k = kf.unflatten(-1, (page, hd // _X, _X))                              # [page][hd]
    else:
        k = kf.unflatten(-1, (hd // _X, page, _X)).permute(0, 1, 3, 2, 4)       # [hd/x][page][x]
    if layout == KV_LAYOUT_REF_VVEC:
        v = vf.unflatten(-1, (page // _X, hd, _X)).permute(0, 1, 2, 4, 3)       # [page/x][hd][x]
    else:
        v = vf.unflatten(-1, (hd, page // _X, _X)).permute(0, 1, 3, 4, 2)       # [hd][page]
    return k, v


def write_tokens(kv_base: torch.Tensor, scale_base: Optional[torch.Tensor], block_table_row: torch.Tensor, start: int,
                 K: torch.Tensor, V: torch.Tensor, k_scale: Optional[torch.Tensor] = None,
                 v_scale: Optional[torch.Tensor] = None, layout: int = KV_LAYOUT_NATIVE) -> None:
    """Store tokens start..start+T-1 of one sequence.  K, V: [T, nkv, hd] in the cache dtype;
    k_scale, v_scale: [T, nkv] fp32 for an int8 cache.  layout: KV_LAYOUT_* of the cache."""
    page = kv_base.shape[3]
    T = K.shape[0]
    pos = torch.arange(start, start + T, device=kv_base.device)
    blk = block_table_row.to(kv_base.device).long()[pos // page]
    off = pos % page
    kview, vview = _natural_views(kv_base, layout)
    K, V = K.to(kv_base.device), V.to(kv_base.device)
    if kv_base.dtype == torch.int8:
        K, V = _flip(K), _flip(V)
    kview[blk, :, off] = K.unflatten(-1, (-1, _X))
    vview[blk, :, off // _X, off % _X, :] = V
    if scale_base is not None:
        scale_base[blk, 0, :, off] = k_scale.to(kv_base.device)
        scale_base[blk, 1, :, off] = v_scale.to(kv_base.device)


def read_tokens(kv_base: torch.Tensor, scale_base: Optional[torch.Tensor], block_table_row: torch.Tensor, ctx: int,
                layout: int = KV_LAYOUT_NATIVE):
    """Natural view of the first ctx tokens of one sequence: (K, V [ctx,nkv,hd], k_scale, v_scale [ctx,nkv] or None)."""
    page = kv_base.shape[3]
    pos = torch.arange(ctx, device=kv_base.device)
    blk = block_table_row.to(kv_base.device).long()[pos // page]
    off = pos % page
    kview, vview = _natural_views(kv_base, layout)
    K, V = kview[blk, :, off].flatten(-2), vview[blk, :, off // _X, off % _X, :]
    if scale_base is None:
        return K, V, None, None
    return _flip(K), _flip(V), scale_base[blk, 0, :, off], scale_base[blk, 1, :, off]


def convert_layout(kv_base: torch.Tensor, src: int, dst: int) -> torch.Tensor:
    """The same logical cache (every token of every block, written or not) as a new tensor in layout `dst`, given `kv_base` in
    layout `src`.  A bijection on the bytes of each head's region; the nominal shape [blocks, 2, nkv, page, hd] is kept."""
    out = torch.empty_like(kv_base)
    ks, vs = _natural_views(kv_base, src)
    kd, vd = _natural_views(out, dst)
    kd.copy_(ks)
    vd.copy_(vs)
    return out
