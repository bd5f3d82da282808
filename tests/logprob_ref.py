"""Reference side of the log-probability tests (mi355_logprobs, mi355_decoder_set_logprobs): the float64 log-softmax and top-N of the
fp32 scaled logits.  The scaled logits come from oracle.apply_penalties, as in sample_ref.scaled_logits (the fp32 multiply by
1 / (T + 1e-6) is part of the semantics); everything after it is float64.  A NaN entry counts as -inf.

Tolerance of a device value against the reference: |dev - ref| <= ABS_TOL + REL_TOL |ref|.  ABS_TOL = 1e-5 is sample_ref.DELTA, the
project's bound for a 152064-term fp32 sum plus the exp rounding: a relative error of the sum is an absolute error of its log.
REL_TOL = 2^-22 is two fp32 roundings of the result (lse = M + log S, lp = x - lse)."""
import numpy as np
import torch

from tests import sample_ref as sr

ABS_TOL = sr.DELTA
REL_TOL = 2.0 ** -22
MIN_GAP = 1e-3        # neighbours among the reference's top N + 1 values must differ by this much before ids are compared exactly


def scaled(logits, temperature=None):
    """[R, V] float64 view of the fp32 scaled logits, NaN as -inf."""
    x = sr.scaled_logits(logits, temperature)
    return np.where(np.isnan(x), -np.inf, x)


def reference(logits, temperature=None, ids=None, top_n=0):
    """-> dict: x [R, V], lse [R], lp [R, V], token [R] (with ids; NaN for an id outside the row), top_ids [R, top_n] (-1 padded),
    top_lp [R, top_n] (-inf padded), gap [R]: the smallest difference between neighbours among the top_n + 1 largest values."""
    x = scaled(logits, temperature)
    R, V = x.shape
    M = x.max(axis=1)
    lse = M + np.log(np.exp(x - M[:, None]).sum(axis=1))
    lp = x - lse[:, None]
    out = {"x": x, "lse": lse, "lp": lp}
    if ids is not None:
        ids = np.asarray(torch.as_tensor(ids).cpu(), dtype=np.int64)
        ok = (ids >= 0) & (ids < V)
        out["token"] = np.where(ok, lp[np.arange(R), np.clip(ids, 0, V - 1)], np.nan)
    top_ids = np.full((R, top_n), -1, dtype=np.int64)
    top_lp = np.full((R, top_n), -np.inf)
    gap = np.full(R, np.inf)
    for r in range(R):
        order = np.argsort(-x[r], kind="stable")               # descending, equal values in index order
        order = order[x[r][order] > -np.inf]
        n = min(top_n, len(order))
        top_ids[r, :n] = order[:n]
        top_lp[r, :n] = lp[r, order[:n]]
        head = x[r][order[: top_n + 1]]
        if len(head) > 1:
            gap[r] = float(np.min(head[:-1] - head[1:]))
    out.update(top_ids=top_ids, top_lp=top_lp, gap=gap)
    return out


def assert_close(dev, ref, what=""):
    """Every device value inside the tolerance of its reference value; infinities and NaN must agree exactly.  Returns the largest
    |dev - ref| / tolerance seen (for reports)."""
    dev = np.asarray(torch.as_tensor(dev).cpu(), dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), f"{what}: NaN pattern differs"
    inf = np.isinf(ref)
    assert np.array_equal(dev[inf], ref[inf]), f"{what}: infinities differ"
    if not fin.any():
        return 0.0
    err = np.abs(dev[fin] - ref[fin])
    ratio = err / (ABS_TOL + REL_TOL * np.abs(ref[fin]))
    worst = int(np.argmax(ratio))
    assert ratio[worst] <= 1.0, f"{what}: |dev - ref| = {err[worst]:.3g} is {ratio[worst]:.2f} of the tolerance (ref {ref[fin][worst]:.6g})"
    return float(ratio[worst])
