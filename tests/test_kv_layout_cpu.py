"""KV block layouts without a GPU: the host codec (kvcache.py) against the permutes the golden generator feeds the reference's own
run_native with (oracle/gen_golden.py: K [blocks, nkv, hd/x, block, x], V [blocks, nkv, hd, block]), the ABI of the `layout` field, the
host-side preparation of the prefill impl and the registration of both impls with reference-shaped plug-in lists.
"""
import ctypes
import itertools

import pytest
import torch

from rtp_llm_amd import _C, attention, kvcache, reference_plugin

NATIVE, REF, VVEC = _C.KV_LAYOUT_NATIVE, _C.KV_LAYOUT_REF, _C.KV_LAYOUT_REF_VVEC
LAYOUTS = [NATIVE, REF, VVEC]


def _natural(nblk, page, nkv, hd, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(nblk * page, nkv, hd, generator=g).to(dtype), torch.randn(nblk * page, nkv, hd, generator=g).to(dtype))


# ------------------------------------------------------------------ 1. codec == the golden generator's expressions
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("page", [16, 64])
def test_codec_writes_the_golden_generators_layouts(dtype, hd, page):
    nblk, nkv, x = 3, 2, 8
    Kn, Vn = _natural(nblk, page, nkv, hd, dtype, hd + page)
    bt = torch.arange(nblk, dtype=torch.int32)                 # identity table: block b holds tokens b * page ..
    k_ref = Kn.view(nblk, page, nkv, hd // x, x).permute(0, 2, 3, 1, 4).reshape(nblk, -1)
    v_lin = Vn.view(nblk, page, nkv, hd).permute(0, 2, 3, 1).reshape(nblk, -1)
    v_vec = Vn.view(nblk, page // x, x, nkv, hd).permute(0, 3, 1, 4, 2).reshape(nblk, -1)
    k_nat = Kn.view(nblk, page, nkv, hd).permute(0, 2, 1, 3).reshape(nblk, -1)
    for layout, ek, ev in ((REF, k_ref, v_lin), (VVEC, k_ref, v_vec), (NATIVE, k_nat, v_lin)):
        kv, _ = kvcache.alloc_layer_cache(nblk, nkv, page, hd, False, "cpu", dtype)
        kvcache.write_tokens(kv, None, bt, 0, Kn, Vn, layout=layout)
        halves = kv.view(nblk, 2, -1)
        assert torch.equal(halves[:, 0], ek), ("K", layout)
        assert torch.equal(halves[:, 1], ev), ("V", layout)


def test_header_offsets_match_the_codec():
    """The offset table of include/mi355_decode.h (what the kernels compute), element by element against the codec."""
    nblk, nkv, page, hd, x = 1, 1, 32, 64, 8
    Kn = torch.arange(page * hd, dtype=torch.float16).view(page, nkv, hd)       # value = t * hd + d, exact in fp16 up to 2048
    for layout in LAYOUTS:
        kv, _ = kvcache.alloc_layer_cache(nblk, nkv, page, hd, False, "cpu")
        kvcache.write_tokens(kv, None, torch.zeros(1, dtype=torch.int32), 0, Kn, Kn, layout=layout)
        kf, vf = kv.view(2, -1)[0], kv.view(2, -1)[1]
        for t, d in itertools.product(range(page), range(hd)):
            ko = t * hd + d if layout == NATIVE else ((d // x) * page + t) * x + d % x
            vo = ((t // x) * hd + d) * x + t % x if layout == VVEC else d * page + t
            assert float(kf[ko]) == t * hd + d and float(vf[vo]) == t * hd + d, (layout, t, d)


# ------------------------------------------------------------------ 2. round trips and conversion
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_read_write_round_trip_and_convert_layout_bijection(dtype):
    nblk, nkv, page, hd, T = 5, 2, 16, 64, 70
    Kn, Vn = _natural(nblk, page, nkv, hd, dtype, 7)
    Kn, Vn = Kn[:T], Vn[:T]
    bt = torch.tensor([3, 0, 4, 1, 2], dtype=torch.int32)      # permuted block table
    caches = {}
    for layout in LAYOUTS:
        kv, _ = kvcache.alloc_layer_cache(nblk, nkv, page, hd, False, "cpu", dtype)
        kvcache.write_tokens(kv, None, bt, 0, Kn[:33], Vn[:33], layout=layout)
        kvcache.write_tokens(kv, None, bt, 33, Kn[33:], Vn[33:], layout=layout)         # a second call that starts inside a page
        K, V, ks, vs = kvcache.read_tokens(kv, None, bt, T, layout=layout)
        assert ks is None and vs is None and torch.equal(K, Kn) and torch.equal(V, Vn), layout
        caches[layout] = kv
    assert not torch.equal(caches[NATIVE], caches[REF]) and not torch.equal(caches[REF], caches[VVEC])
    for a, b in itertools.permutations(LAYOUTS, 2):            # all six pairs
        ab = kvcache.convert_layout(caches[a], a, b)
        assert ab.shape == caches[a].shape and ab.dtype == dtype
        assert torch.equal(ab, caches[b]), (a, b)               # agrees with write-then-read in the other layout
        assert torch.equal(kvcache.convert_layout(ab, b, a), caches[a]), (a, b)
    # the whole tensor takes part, written or not
    junk = torch.randn(nblk, 2, nkv, page, hd).to(dtype)
    assert torch.equal(kvcache.convert_layout(kvcache.convert_layout(junk, NATIVE, VVEC), VVEC, NATIVE), junk)


def test_codec_refuses_int8_in_a_reference_layout_and_unknown_layouts():
    kv, sc = kvcache.alloc_layer_cache(2, 1, 16, 64, True, "cpu")
    with pytest.raises(ValueError):
        kvcache.read_tokens(kv, sc, torch.zeros(1, dtype=torch.int32), 4, layout=REF)
    kv16, _ = kvcache.alloc_layer_cache(2, 1, 16, 64, False, "cpu")
    with pytest.raises(ValueError):
        kvcache.convert_layout(kv16, NATIVE, 7)


# ------------------------------------------------------------------ 3. ABI
def test_abi_layout_field_setter_and_argument_errors_without_a_device():
    assert [n for n, _ in _C.KVLayer._fields_][-1] == "layout"
    kv = _C.KVLayer(1, None, _C.KV_FP16, 16, 4, 128, 8)        # positional construction without the field stays native
    assert kv.layout == _C.KV_LAYOUT_NATIVE == 0 and (REF, VVEC) == (1, 2)
    assert ctypes.sizeof(_C.KVLayer) == 48
    l = _C.lib()
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), "mi355_decoder_set_kv_layout")
    assert l.mi355_decoder_set_kv_layout(None, REF) == _C.ERR_ARG
    # argument errors come from the host, before any launch: the pointers are never touched
    for kvd, layout, word in ((_C.KV_INT8, REF, b"INT8"), (_C.KV_INT8, VVEC, b"INT8"), (_C.KV_FP16, 7, b"unknown"), (_C.KV_BF16, -1, b"unknown")):
        kv = _C.KVLayer(1, 1, kvd, 16, 4, 128, 8, _C.ACT_BF16 if kvd == _C.KV_BF16 else _C.ACT_F16, layout)
        assert l.mi355_paged_decode_attn(1, ctypes.byref(kv), 1, 4, 1, 1, 28, 0.1, 64, 1, None, 0, None) == _C.ERR_ARG
        assert word in l.mi355_last_error(), l.mi355_last_error()
        assert l.mi355_rope_kv_write(1, None, 0, 36 * 128, None, 1, 128, 64, 1, 1, 4, 1, 28, ctypes.byref(kv), 1, None, None) == _C.ERR_ARG
        assert word in l.mi355_last_error(), l.mi355_last_error()
        assert l.mi355_paged_attn_rows(1, ctypes.byref(kv), 1, 4, 1, 1, 2, 28, 0.1, 64, 1, None, 0, None) == _C.ERR_ARG
        assert l.mi355_paged_attn_rows_img(1, ctypes.byref(kv), 1, 4, 1, 1, 2, 28, 0.1, 64, 1, None, 0, None) == _C.ERR_ARG
    # a reference layout with a page it does not exist for
    kv = _C.KVLayer(1, None, _C.KV_FP16, 24, 4, 128, 8, _C.ACT_F16, REF)
    assert l.mi355_paged_decode_attn(1, ctypes.byref(kv), 1, 4, 1, 1, 28, 0.1, 64, 1, None, 0, None) == _C.ERR_ARG
    assert b"page" in l.mi355_last_error()


# ------------------------------------------------------------------ 4. prefill impl, host side
def _cfg(**kw):
    base = dict(head_num=8, kv_head_num=2, size_per_head=64, rope_dim=64, max_seq_len=64)
    base.update(kw)
    return attention.AttentionConfigs(**base)


def test_prefill_impl_support_truth_table():
    pre, dec = attention.PyAttentionInputs(is_prefill=True), attention.PyAttentionInputs(is_prefill=False)
    P, D = attention.Mi355PrefillImpl, attention.Mi355PagedDecodeImpl
    assert P.support(_cfg(), pre) and not P.support(_cfg(), dec)
    assert D.support(_cfg(), dec) and not D.support(_cfg(), pre)
    for bad in (dict(size_per_head=96, rope_dim=96), dict(head_num=34, kv_head_num=2), dict(head_num=8, kv_head_num=3), dict(rope_dim=32)):
        assert not P.support(_cfg(**bad), pre), bad
        assert not D.support(_cfg(**bad), dec), bad
    assert P.support(_cfg(rope_dim=0), pre) and P.support(_cfg(size_per_head=128, rope_dim=128, head_num=16, kv_head_num=1), pre)
    assert attention.PyAttentionInputs().prefix_lengths is None and attention.PyAttentionInputs().cu_seqlens is None
    assert _cfg().kv_layout == NATIVE
    assert attention.PREFILL_MHA_IMPS == [P] and attention.DECODE_MHA_IMPS == [D]


def test_prefill_impl_prepare_builds_the_padded_row_layout():
    lens, prefix = [5, 1, 16], [0, 16, 3]
    ai = attention.PyAttentionInputs(True, None, torch.tensor(lens, dtype=torch.int32), torch.arange(12, dtype=torch.int32).reshape(3, 4),
                                     prefix_lengths=torch.tensor(prefix, dtype=torch.int32), cu_seqlens=torch.tensor([0, 5, 6, 22], dtype=torch.int32))
    impl = attention.AttnImplFactory.get_fmha_impl(_cfg(), ai)
    assert type(impl) is attention.Mi355PrefillImpl
    q_len, T = 16, 22
    assert (impl.batch, impl.q_len, impl.num_tokens) == (3, q_len, T)
    want_pos = torch.full((3 * q_len,), -1, dtype=torch.int32)
    want_pos[0:5] = torch.arange(0, 5, dtype=torch.int32)
    want_pos[16:17] = 16
    want_pos[32:48] = torch.arange(3, 19, dtype=torch.int32)
    assert impl.positions.dtype == torch.int32 and torch.equal(impl.positions, want_pos)
    want_rows = torch.tensor(list(range(0, 5)) + [16] + list(range(32, 48)))
    assert torch.equal(impl.row_of_token, want_rows)
    want_tok = torch.full((3 * q_len,), -1, dtype=torch.int64)
    want_tok[want_rows] = torch.arange(T)
    assert torch.equal(impl.token_of_row, want_tok)
    assert impl.block_table.dtype == torch.int32 and impl.block_table.shape == (3, 4)
    packed = torch.randn(T, 6).half()
    padded = impl.scatter(packed)
    assert padded.shape == (48, 6) and torch.equal(padded[impl.token_of_row < 0], torch.zeros(48 - T, 6).half())
    assert torch.equal(padded[want_rows], packed)
    assert torch.equal(impl.gather(padded), packed)            # scatter then gather: the identity on the packed rows
    # cu_seqlens alone describes the batch as well
    ai2 = attention.PyAttentionInputs(True, None, None, ai.kv_cache_kernel_block_id_device, cu_seqlens=ai.cu_seqlens)
    impl2 = attention.Mi355PrefillImpl(_cfg(), ai2)
    assert impl2.q_len == 16 and torch.equal(impl2.row_of_token, want_rows) and int(impl2.positions[16]) == 0
    with pytest.raises(ValueError):                            # 60 cached + 16 new > max_seq_len 64
        attention.Mi355PrefillImpl(_cfg(), attention.PyAttentionInputs(True, None, ai.input_lengths, ai.kv_cache_kernel_block_id_device,
                                                                       prefix_lengths=torch.tensor([0, 0, 60], dtype=torch.int32)))


# ------------------------------------------------------------------ 5. registration with reference-shaped lists
def test_register_attention_binds_both_impls_to_the_given_base():
    class StubBase:                                            # stands for the reference's FMHAImplBase
        marker = "reference base"

    class Other(StubBase):
        @staticmethod
        def support(attn_configs, attn_inputs):
            return True

    decode_list, prefill_list = [Other], [Other]
    out = reference_plugin.register_attention(decode_list, prefill_list, StubBase)
    assert len(out) == 2 and decode_list[0] is out[0] and prefill_list[0] is out[1]
    assert decode_list[1] is Other and prefill_list[1] is Other and len(decode_list) == len(prefill_list) == 2
    assert issubclass(out[0], StubBase) and issubclass(out[0], attention.Mi355PagedDecodeImpl)
    assert issubclass(out[1], StubBase) and issubclass(out[1], attention.Mi355PrefillImpl)
    assert out[0].marker == out[1].marker == "reference base"

    def first_match(lst, ai):                                  # attn_factory.py:226-254
        return next(c for c in lst if c.support(_cfg(), ai))
    dec, pre = attention.PyAttentionInputs(is_prefill=False), attention.PyAttentionInputs(is_prefill=True)
    assert first_match(decode_list, dec) is out[0] and first_match(prefill_list, pre) is out[1]
    # an unsupported head shape falls through to the next registered impl, as in the reference's factory
    assert next(c for c in decode_list if c.support(_cfg(size_per_head=96, rope_dim=96), dec)) is Other
    # the package's own lists are untouched
    assert attention.DECODE_MHA_IMPS == [attention.Mi355PagedDecodeImpl] and attention.PREFILL_MHA_IMPS == [attention.Mi355PrefillImpl]
