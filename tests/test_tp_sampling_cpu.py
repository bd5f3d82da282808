"""Host side of sampled decoding and log-probabilities under tensor parallelism: the sizes of the gathered-logits buffer, argument
validation of the new entry points before anything is launched, the arithmetic of distributed.logits_gather_bytes, and the condition on
the reference that tests/test_gpu_tp_sampling.py relies on.  Runs with -m "not gpu"."""
import ctypes

import numpy as np
import pytest
import torch

from rtp_llm_amd import _C, distributed
from tests import sample_ref as sr
from tests import tp_sampling_cases as tc


def _mc(tp, max_batch=5, vocab=512):
    return _C.ModelConfig(2, 512, 4, 1, 64, 384, vocab, 64, 256, 1e-6, _C.KV_FP16, 16, 10, max_batch, 2, 32, tp, _C.ACT_F16)


def test_gathered_logits_bytes():
    l = _C.lib()
    assert l.mi355_decoder_gathered_logits_bytes(None) == 0
    assert l.mi355_decoder_gathered_logits_bytes(ctypes.byref(_mc(1))) == 0
    for tp, mb, v in ((2, 5, 512), (8, 64, 19008), (8, 3, 16032)):
        n = l.mi355_decoder_gathered_logits_bytes(ctypes.byref(_mc(tp, mb, v)))
        assert n >= mb * tp * v * 4 and n % 256 == 0, (tp, mb, v, n)
    # the tail's workspaces cover tp * vocab columns under tensor parallelism and are what they were at tp 1
    one, two = _mc(1, 5, 1024), _mc(2, 5, 512)
    assert l.mi355_decoder_sampling_workspace_bytes(ctypes.byref(two)) == l.mi355_decoder_sampling_workspace_bytes(ctypes.byref(one))
    assert l.mi355_decoder_logprobs_workspace_bytes(ctypes.byref(two), 3) == l.mi355_decoder_logprobs_workspace_bytes(ctypes.byref(one), 3)
    pen = (5 * 1024 * 4 + 255) // 256 * 256
    assert l.mi355_decoder_sampling_workspace_bytes(ctypes.byref(one)) == pen + (l.mi355_sample_logits_workspace_bytes(5, 1024) + 255) // 256 * 256


def test_new_entry_points_validate_on_the_host():
    l = _C.lib()
    assert l.mi355_decoder_set_gathered_logits(None, 256, 1 << 20) == _C.ERR_ARG and b"decoder is null" in l.mi355_last_error()
    assert l.mi355_decoder_set_gathered_logits(None, None, 0) == _C.ERR_ARG and b"decoder is null" in l.mi355_last_error()
    assert l.mi355_allgather_logits(None, 256, 512, 4096, 4, 512, None) == _C.ERR_ARG and b"not opened" in l.mi355_last_error()
    assert l.mi355_allgather_logits(None, None, 512, None, 4, 512, None) == _C.ERR_ARG and b"not opened" in l.mi355_last_error()


def test_logits_gather_bytes_arithmetic():
    unit = distributed.LOGITS_GATHER_UNIT
    assert unit == 4096
    assert distributed.logits_gather_bytes(1, 4) == unit                          # one unit is the least a context can hold
    assert distributed.logits_gather_bytes(1, 1024) == unit                       # exactly one
    assert distributed.logits_gather_bytes(1, 1028) == 2 * unit                   # one vector more
    assert distributed.logits_gather_bytes(64, 516) == (64 * 516 * 4 + unit - 1) // unit * unit == 33 * unit
    for B, V in ((5, 1000), (3, 37988), (64, 19008)):
        n = distributed.logits_gather_bytes(B, V)
        assert n % unit == 0 and 0 <= n - B * V * 4 < unit
    with pytest.raises(ValueError):
        distributed.logits_gather_bytes(0, 512)


def test_the_reference_separates_the_bands_of_the_sampled_steps_first_rows():
    """tests/test_gpu_tp_sampling.py checks step 0 of its sampled step with sample_ref.check_rows(k_band=True), whose reference asserts
    that at most sample_ref.MAX_FREE entries of a row stay undecided.  The weights' seed is chosen so that the reference alone meets
    that on the oracle's logits of the same step (row_reference raises otherwise), with room to spare for the kernels' 1e-2."""
    rows = tc.oracle_step0_rows(tc.weights())
    x = sr.scaled_logits(rows, torch.tensor(tc.PARAMS["temperature"]))
    assert x.shape == (tc.B, tc.CFG.vocab) and np.isfinite(x).all()
    for r in range(tc.B):
        k, p = tc.PARAMS["top_k"][r], tc.PARAMS["top_p"][r]
        if k == 1:
            continue
        _, keep, drop = sr.row_reference(x[r], k, p, k_band=True)
        assert (~(keep | drop)).sum() <= sr.MAX_FREE // 2, r
        assert keep.sum() >= 2, (r, int(keep.sum()))                              # a real choice is left: the draw is not a disguised arg-max
