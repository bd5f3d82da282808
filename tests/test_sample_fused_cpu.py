"""Host side of the fused sampling tail (mi355_sample_logits, mi355_apply_penalties_history, mi355_decoder_set_sampling): the tests'
numpy Philox against the Random123 known answers, and argument validation before anything is launched.  Runs with -m "not gpu"."""
import ctypes

import numpy as np

from rtp_llm_amd import _C
from tests import sample_ref as sr


def _words(s):
    return [int(w, 16) for w in s.split()]


def test_numpy_philox_reproduces_random123_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds."""
    kat = [("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = sr.philox4x32_10(_words(ctr), _words(key))[0]
        assert [int(v) for v in got] == _words(want), (ctr, key, [hex(int(v)) for v in got])
    # batched form, and the uniform of (seed, position): key = the seed's two words, counter = (position, 0, 0, 0)
    both = sr.philox4x32_10([_words(kat[0][0]), _words(kat[2][0])], [_words(kat[0][1]), _words(kat[2][1])])
    assert [int(v) for v in both[1]] == _words(kat[2][2])
    u = sr.philox_uniform([0, (0x299f31d0 << 32) | 0xa4093822], [0, 7])
    assert u[0] == np.float32((0x6627e8d5 >> 8) * 2.0 ** -24)
    x0 = sr.philox4x32_10([7, 0, 0, 0], [0xa4093822, 0x299f31d0])[0, 0]
    assert u[1] == np.float32((int(x0) >> 8) * 2.0 ** -24) and 0.0 <= u[1] < 1.0


def test_sample_logits_validates_on_the_host():
    l = _C.lib()
    need = l.mi355_sample_logits_workspace_bytes(2, 10)
    assert need > 0 and l.mi355_sample_logits_workspace_bytes(64, 152064) == l.mi355_sample_logits_workspace_bytes(64, 97)
    ok = lambda *a: l.mi355_sample_logits(*a)
    #            logits rows V ld  temp  k     p     u     seed  pos   ids   u_out p_out ld_out ws   bytes stream
    assert ok(None, 0, 10, 10, None, None, None, None, None, None, None, None, None, 0, None, 0, None) == 0          # rows == 0
    assert ok(None, 2, 10, 10, None, None, None, 1, None, None, 1, None, None, 0, 8, need, None) == _C.ERR_ARG
    assert b"logits" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, None, 1, None, None, None, None, None, 0, 8, need, None) == _C.ERR_ARG
    assert b"ids" in l.mi355_last_error()
    assert ok(1, 2, 10, 8, None, None, None, 1, None, None, 1, None, None, 0, 8, need, None) == _C.ERR_ARG
    assert b"ld" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, None, None, None, None, 1, None, None, 0, 8, need, None) == _C.ERR_ARG            # neither uniforms nor seed
    assert b"uniform_samples" in l.mi355_last_error() and b"seed" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, None, None, 1, None, 1, None, None, 0, 8, need, None) == _C.ERR_ARG               # a seed without positions
    assert b"draw_positions" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, None, 1, None, None, 1, None, 1, 8, 8, need, None) == _C.ERR_ARG                  # ld_out < V
    assert b"ld_out" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, None, 1, None, None, 1, None, None, 0, 8, need - 1, None) == _C.ERR_WORKSPACE
    assert b"workspace" in l.mi355_last_error()
    assert ok(1, 2, 10, 10, None, None, None, 1, None, None, 1, None, None, 0, None, 0, None) == _C.ERR_WORKSPACE


def test_penalties_history_and_set_sampling_validate_on_the_host():
    l = _C.lib()
    pen = lambda *a: l.mi355_apply_penalties_history(*a)
    #              logits rows V ld  rep   pres  freq  hist  ld len   ws   stream
    assert pen(None, 0, 10, 10, None, None, None, None, 0, None, None, None) == 0
    assert pen(None, 2, 10, 10, 1, None, None, 1, 4, 1, 1, None) == _C.ERR_ARG and b"logits" in l.mi355_last_error()
    assert pen(1, 2, 10, 8, 1, None, None, 1, 4, 1, 1, None) == _C.ERR_ARG and b"ld" in l.mi355_last_error()
    assert pen(1, 2, 10, 10, 1, None, None, None, 4, None, 1, None) == _C.ERR_ARG and b"history" in l.mi355_last_error()   # penalties without a history
    assert pen(1, 2, 10, 10, None, 1, None, 1, 4, None, 1, None) == _C.ERR_ARG and b"history_len" in l.mi355_last_error()
    assert pen(1, 2, 10, 10, None, None, 1, 1, 4, 1, None, None) == _C.ERR_ARG and b"penalty_ws" in l.mi355_last_error()
    assert pen(1, 2, 10, 10, None, None, None, None, 0, None, None, None) == 0                                               # nothing to apply
    s = _C.Sampling()
    assert l.mi355_decoder_set_sampling(None, ctypes.byref(s)) == _C.ERR_ARG and b"decoder" in l.mi355_last_error()
    assert l.mi355_decoder_set_sampling(None, None) == _C.ERR_ARG
    assert l.mi355_decoder_sampling_workspace_bytes(None) == 0
    mc = _C.ModelConfig(2, 512, 8, 2, 64, 1024, 2048, 64, 512, 1e-6, _C.KV_FP16, 16, 64, 8, 8, 128, 1, _C.ACT_F16)
    assert l.mi355_decoder_sampling_workspace_bytes(ctypes.byref(mc)) >= 8 * 2048 * 4 + l.mi355_sample_logits_workspace_bytes(8, 2048)
