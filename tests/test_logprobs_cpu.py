"""Host side of the log-probability path (mi355_logprobs, mi355_decoder_set_logprobs): the tests' float64 reference against torch, and
argument validation before anything is launched.  Runs with -m "not gpu"."""
import ctypes

import numpy as np
import torch

from rtp_llm_amd import _C
from tests import logprob_ref as lr


def test_reference_equals_torch_log_softmax_and_topk_in_float64():
    g = torch.Generator().manual_seed(5)
    for V, scale in ((5, 1.0), (1003, 4.0), (32003, 20.0)):
        logits = torch.randn(3, V, generator=g) * scale
        logits[0, V // 2] = float("-inf")
        logits[1, V // 3] = float("nan")                       # counts as -inf
        temp = torch.tensor([0.7, 1.0, 1.9])
        ids = torch.tensor([0, V // 3, V - 1])
        n = 4
        ref = lr.reference(logits, temp, ids, n)
        x = torch.from_numpy(ref["x"])
        want = torch.log_softmax(x, dim=1)
        assert np.allclose(ref["lp"], want.numpy(), rtol=0, atol=1e-12, equal_nan=True)
        assert np.allclose(ref["lse"], torch.logsumexp(x, dim=1).numpy(), rtol=0, atol=1e-12)
        tv, ti = torch.topk(x, n, dim=1)                      # random values: no ties
        assert np.array_equal(ref["top_ids"], ti.numpy())
        assert np.allclose(ref["top_lp"], (tv - torch.logsumexp(x, dim=1, keepdim=True)).numpy(), rtol=0, atol=1e-12)
        assert ref["token"][1] == -np.inf and np.isfinite(ref["token"][[0, 2]]).all()
        assert (ref["gap"] > 0).all()
    # equal values in index order, padding, an id outside the row
    ref = lr.reference(torch.tensor([[1.0, 2.0, 2.0, float("-inf"), 2.0]]), None, torch.tensor([7]), 6)
    assert ref["top_ids"].tolist() == [[1, 2, 4, 0, -1, -1]] and np.isnan(ref["token"][0]) and ref["gap"][0] == 0.0
    assert ref["top_lp"][0, 4] == -np.inf
    # the tolerance helper: inside, outside, infinities
    lr.assert_close(torch.tensor([-1.0 + 5e-6, float("-inf")]), np.array([-1.0, -np.inf]))
    for bad in ([-1.0 + 3e-5, float("-inf")], [-1.0, -50.0]):
        try:
            lr.assert_close(torch.tensor(bad), np.array([-1.0, -np.inf]))
        except AssertionError:
            continue
        raise AssertionError("assert_close accepted a value outside the tolerance")


def test_logprobs_validates_on_the_host():
    l = _C.lib()
    need = l.mi355_logprobs_workspace_bytes(2, 10, 4)
    assert need > 0
    # the workspace does not depend on V
    assert l.mi355_logprobs_workspace_bytes(64, 152064, 20) == l.mi355_logprobs_workspace_bytes(64, 97, 20)
    assert l.mi355_logprobs_workspace_bytes(64, 152064, 0) < l.mi355_logprobs_workspace_bytes(64, 152064, 32)
    ok = lambda *a: l.mi355_logprobs(*a)
    #         logits rows V ld  temp  ids   n  tok   lse   t_ids t_lp  top_ld ws  bytes stream
    assert ok(None, 0, 10, 10, None, None, 0, None, None, None, None, 0, None, 0, None) == 0                 # rows == 0
    assert ok(None, 2, 10, 10, None, None, 0, None, 1, None, None, 0, 8, need, None) == _C.ERR_ARG
    assert b"logits" in l.mi355_last_error()
    assert ok(1, 2, 10, 8, None, None, 0, None, 1, None, None, 0, 8, need, None) == _C.ERR_ARG
    assert b"ld" in l.mi355_last_error()
    for n in (-1, 33):
        assert ok(1, 2, 10, 10, None, None, n, None, 1, 1, 1, 40, 8, need, None) == _C.ERR_ARG
        assert b"top_n" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, 1, 0, None, 1, None, None, 0, 8, need, None) == _C.ERR_ARG                 # ids without token_logprobs
    assert b"token_logprobs" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, 4, None, 1, None, 1, 4, 8, need, None) == _C.ERR_ARG                 # top_n without top_ids
    assert b"top_ids" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, 4, None, 1, 1, None, 4, 8, need, None) == _C.ERR_ARG                 # ... without top_logprobs
    assert b"top_logprobs" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, 4, None, 1, 1, 1, 3, 8, need, None) == _C.ERR_ARG                    # top_ld < top_n
    assert b"top_ld" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, 1, 4, 1, 1, 1, 1, 4, 8, need - 1, None) == _C.ERR_WORKSPACE
    assert b"workspace" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, 1, 4, 1, 1, 1, 1, 4, None, 0, None) == _C.ERR_WORKSPACE
    assert _C.LOGPROBS_MAX_TOP == 32


def test_set_logprobs_validates_on_the_host():
    l = _C.lib()
    lp = _C.Logprobs()
    assert l.mi355_decoder_set_logprobs(None, ctypes.byref(lp)) == _C.ERR_ARG and b"decoder" in l.mi355_last_error()
    assert l.mi355_decoder_set_logprobs(None, None) == _C.ERR_ARG
    assert l.mi355_decoder_logprobs_workspace_bytes(None, 4) == 0
    mc = _C.ModelConfig(2, 512, 8, 2, 64, 1024, 2048, 64, 512, 1e-6, _C.KV_FP16, 16, 64, 8, 8, 128, 1, _C.ACT_F16)
    assert l.mi355_decoder_logprobs_workspace_bytes(ctypes.byref(mc), 20) >= l.mi355_logprobs_workspace_bytes(8, 2048, 20) > 0
