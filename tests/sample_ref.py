"""Reference side of the fused sampling tail's tests (mi355_sample_logits): a numpy Philox4x32-10 and the float64 band checks of the
kept set, the renormalised probabilities and the draw.  The scaled logits come from oracle.apply_penalties (the fp32 multiply by
1 / (T + 1e-6) is part of the semantics); everything after it is float64."""
import numpy as np
import torch

from oracle import oracle

DELTA = 1e-5          # slack on the preceding mass (top-p) and on the draw: ~10x the fp32 error of a 152064-term sum + the exp rounding
MAX_FREE = 8          # entries the band may leave undecided per row (a condition on the reference, asserted)
MIN_K_GAP = 1e-3      # k-th and (k+1)-th scaled logits must differ by this much (a condition on the reference, asserted)

_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] uint32 -> [..., 4] uint32 (Random123 philox4x32, 10 rounds)."""
    c = np.array(counter, dtype=np.uint32).copy()
    k = np.array(key, dtype=np.uint32).copy()
    c, k = np.atleast_2d(c), np.atleast_2d(k)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = _M0 * c[:, 0].astype(np.uint64)
            p1 = _M1 * c[:, 2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
            c = np.stack([hi1 ^ c[:, 1] ^ k[:, 0], lo1, hi0 ^ c[:, 3] ^ k[:, 1], lo0], axis=1)
            k = np.stack([k[:, 0] + _W0, k[:, 1] + _W1], axis=1)
    return c


def philox_uniform(seeds, positions):
    """u = (x0 >> 8) * 2^-24 for key = (seed low word, seed high word), counter = (position, 0, 0, 0); seeds as unsigned 64-bit ints."""
    s = np.asarray(seeds, dtype=np.uint64).reshape(-1)
    pos = np.asarray(positions, dtype=np.int64).reshape(-1).astype(np.uint32)
    key = np.stack([(s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)], axis=1)
    ctr = np.zeros((len(s), 4), dtype=np.uint32)
    ctr[:, 0] = pos
    x0 = philox4x32_10(ctr, key)[:, 0]
    return ((x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def seeds_as_int64(seeds):
    """unsigned 64-bit seeds -> the int64 tensor holding the same bit patterns (what ops.sample_logits / the engine take)."""
    return torch.from_numpy(np.asarray(seeds, dtype=np.uint64).view(np.int64).copy())


def scaled_logits(logits, temperature):
    """float64 view of the fp32 scaled logits (temperature as the kernels apply it)."""
    x = logits.detach().cpu().float()
    if temperature is not None:
        x = oracle.apply_penalties(x, temperature=torch.as_tensor(temperature, dtype=torch.float32))
    return x.numpy().astype(np.float64)


def row_reference(x, k, p, ties_ok=False, k_band=False):
    """One row of scaled logits (float64) -> (probs, must_keep, must_drop): the band rule of the kept set.  Asserts the conditions on
    the reference itself: at most MAX_FREE undecided entries, and a clear k-th value (unless ties are the point: then ties stay).
    k_band is for logits that the test does not choose (a model's): where the k-th and (k+1)-th values are closer than MIN_K_GAP the
    entries within MIN_K_GAP of the k-th value are undecided instead, and count towards MAX_FREE like those of the top-p band."""
    V = x.shape[0]
    pr = np.exp(x - x.max())
    pr /= pr.sum()
    order = np.argsort(-x, kind="stable")                 # descending, equal values in index order
    keep_k = np.ones(V, dtype=bool)
    drop_k = np.zeros(V, dtype=bool)
    if 0 < k < V:
        kth = x[order[k - 1]]
        keep_k = x >= kth                                 # ties with the k-th value stay
        if not ties_ok and kth - x[order[k]] < MIN_K_GAP:
            assert k_band, "the reference's k-th and (k+1)-th values are too close for this test"
            keep_k = x >= kth + MIN_K_GAP
            drop_k = x <= kth - MIN_K_GAP
        else:
            drop_k = ~keep_k
    if abs(p) < 1e-7:
        p = 1.0
    if abs(p - 1.0) < 1e-7:
        assert (~(keep_k | drop_k)).sum() <= MAX_FREE, "undecided entries around the k-th value: the inputs do not separate the band"
        return pr, keep_k.copy(), drop_k
    before = np.empty(V)
    cs = np.cumsum(pr[order])
    before[order] = cs - pr[order]                        # mass of the full-vocabulary softmax in front of each entry
    must_keep = keep_k & (before <= p * (1 - DELTA))
    must_drop = drop_k | (before > p * (1 + DELTA))
    free = ~(must_keep | must_drop)
    assert free.sum() <= MAX_FREE, f"{int(free.sum())} undecided entries: the inputs do not separate the band"
    return pr, must_keep, must_drop


def check_rows(logits, temperature, top_k, top_p, u, ids, probs_out, ties_ok=False, report=None, k_band=False):
    """The op-level checks of every row: kept set inside the band, renormalised probabilities, drawn id and its CDF interval."""
    x = scaled_logits(logits, temperature)
    raw = logits.detach().cpu().float().numpy()
    ids = np.asarray(ids.cpu()); out = np.asarray(probs_out.cpu(), dtype=np.float64); u = np.asarray(u.cpu(), dtype=np.float64)
    for r in range(x.shape[0]):
        k = int(top_k[r]) if top_k is not None else 0
        p = float(top_p[r]) if top_p is not None else 1.0
        kept = out[r] > 0
        if k == 1:                                        # greedy row: the arg-max of the raw logits, lowest index on ties
            assert ids[r] == int(np.argmax(raw[r])), f"row {r}: greedy id"
            assert kept.sum() == 1 and kept[ids[r]] and out[r, ids[r]] == 1.0
            continue
        pr, must_keep, must_drop = row_reference(x[r], k, p, ties_ok, k_band)
        assert not (must_keep & ~kept).any(), f"row {r}: dropped {np.flatnonzero(must_keep & ~kept)[:5]} that must stay"
        assert not (must_drop & kept).any(), f"row {r}: kept {np.flatnonzero(must_drop & kept)[:5]} that must go"
        ref = pr * kept / pr[kept].sum()                  # renormalised over the (now validated) kept set
        rel = np.abs(out[r][kept] - ref[kept]) / ref[kept]
        if report is not None:
            report.append((r, int(kept.sum()), float(rel.max())))
        assert rel.max() <= 1e-5, f"row {r}: probs_out off by {rel.max():.3g} (relative)"
        assert kept[ids[r]], f"row {r}: drew a filtered entry"
        cdf = np.cumsum(ref)
        lo = cdf[ids[r]] - ref[ids[r]]
        assert lo - DELTA <= u[r] <= cdf[ids[r]] + DELTA, f"row {r}: u={u[r]} outside [{lo}, {cdf[ids[r]]}] of id {ids[r]}"
        if kept.sum() == 1:
            assert ids[r] == int(np.argmax(raw[r])), f"row {r}: one-token nucleus is not the arg-max"
