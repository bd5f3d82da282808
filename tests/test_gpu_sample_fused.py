"""The fused sampling tail on the GPU, op level (mi355_sample_logits, mi355_apply_penalties_history) against the float64 band reference
of tests/sample_ref.py, the oracle's filter / penalties and the numpy Philox."""
import numpy as np
import pytest
import torch

from oracle import oracle
from rtp_llm_amd import ops
from tests import sample_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SCALES, TEMPS, TOP_PS, TOP_KS = [0.25, 1.0, 2.0, 4.0], [0.7, 1.0, 1.3], [0.5, 0.8, 0.9, 0.95], [0, 20, 50]


def _mixed_rows(V, n_grid, seed):
    """n_grid rows walking the (scale, T, top_p, top_k) grid, then the special rows: top_k = 1, top_k >= V, top_p = 1, top_p = 1e-6."""
    g = torch.Generator().manual_seed(seed)
    scale, temp, tp, tk = [], [], [], []
    for i in range(n_grid):
        scale.append(SCALES[i % 4]); temp.append(TEMPS[(i // 4 + i) % 3]); tp.append(TOP_PS[(i // 2 + i) % 4]); tk.append(TOP_KS[(i // 3) % 3])
    special = [(1.0, 0.7, 0.9, 1), (2.0, 1.3, 0.8, V + 5), (1.0, 1.0, 1.0, 20), (2.0, 0.7, 1e-6, 0), (4.0, 1.0, 1.0, 0), (1.0, 1.3, 0.5, V)]
    for s, t, p, k in special:
        scale.append(s); temp.append(t); tp.append(p); tk.append(k)
    R = len(scale)
    x = torch.randn(R, V, generator=g) * torch.tensor(scale).unsqueeze(1)
    u = torch.rand(R, generator=g)
    return x, torch.tensor(temp), torch.tensor(tk, dtype=torch.int32), torch.tensor(tp), u


@pytest.mark.parametrize("V,ld,n_grid", [(97, 97, 12), (4099, 4104, 12), (152064, 152064, 0)])
def test_kept_set_probabilities_and_draw_against_float64(V, ld, n_grid):
    if V == 152064:      # 4 rows: the flat nucleus of ~90 000 entries, a top-k row, and the two rows that must be the arg-max
        g = torch.Generator().manual_seed(3)
        x = torch.randn(4, V, generator=g) * torch.tensor([1.0, 2.0, 1.0, 4.0]).unsqueeze(1)
        temp, tk = torch.tensor([1.0, 0.7, 1.3, 0.7]), torch.tensor([0, 50, 1, 0], dtype=torch.int32)
        tp, u = torch.tensor([0.9, 0.8, 0.9, 1e-6]), torch.rand(4, generator=g)
    else:
        x, temp, tk, tp, u = _mixed_rows(V, n_grid, seed={97: 97, 4099: 2}[V])   # seeds at which the reference's own conditions hold
    buf = torch.full((x.shape[0], ld), float("nan"), device=DEV)       # padding columns hold NaN: never read
    buf[:, :V] = x.to(DEV)
    ids, out = ops.sample_logits(buf[:, :V], temp, tk, tp, uniform=u, return_probs=True)
    report = []
    sr.check_rows(x, temp, tk, tp, u, ids, out, report=report)
    print("rows (row, survivors, max relative error of probs_out):", report)
    if V <= 4099:        # outside the band the oracle's filter keeps the same entries (fp32 statement-for-statement filter)
        probs = torch.softmax(oracle.apply_penalties(x, temperature=temp).double(), -1).float()
        want = oracle.top_k_top_p_filter(probs, tk, tp) > 0
        got = out.cpu() > 0
        for r in range(x.shape[0]):
            if int(tk[r]) == 1:
                continue
            _, must_keep, must_drop = sr.row_reference(sr.scaled_logits(x[r:r + 1], temp[r:r + 1])[0], int(tk[r]), float(tp[r]))
            decided = torch.from_numpy(must_keep | must_drop)
            assert torch.equal(got[r][decided], want[r][decided]), r
    # no filter at all: None for every parameter draws from the plain softmax
    ids0, out0 = ops.sample_logits(buf[:, :V], uniform=u, return_probs=True)
    sr.check_rows(x, None, None, None, u, ids0, out0)


@pytest.mark.parametrize("V", [640, 152064])
def test_ties_stay_with_the_kth_value_and_split_in_index_order(V):
    """Logits from {0..5}: whole runs of equal values.  top_k = V / 3 keeps exactly {x >= k-th value}; top-p cuts inside a run, in index order."""
    g = torch.Generator().manual_seed(V)
    x = torch.randint(0, 6, (3, V), generator=g).float()
    k = V // 3
    tk = torch.tensor([k, k, 0], dtype=torch.int32)
    tp = torch.tensor([1.0, 0.3, 0.7])
    u = torch.rand(3, generator=g)
    ids, out = ops.sample_logits(x.to(DEV), None, tk, tp, uniform=u, return_probs=True)
    kept = out.cpu() > 0
    kth = x[0].sort(descending=True).values[k - 1]
    assert torch.equal(kept[0], x[0] >= kth) and int(kept[0].sum()) > k
    sr.check_rows(x, None, tk, tp, u, ids, out, ties_ok=True)
    for r in (1, 2):     # the cut falls inside a run: of the smallest kept value, the kept entries are the first ones in index order
        v = x[r][kept[r]].min()
        run = torch.nonzero(x[r] == v).flatten()
        n = int(kept[r][run].sum())
        assert 0 < n < len(run) and bool(kept[r][run[:n]].all()) and not bool(kept[r][run[n:]].any()), (r, n, len(run))
        assert bool(kept[r][x[r] > v].all())


def test_philox_uniforms_are_bit_equal_to_numpy_and_explicit_uniforms_override():
    g = np.random.default_rng(11)
    R, V = 33, 97
    seeds = g.integers(0, 2 ** 64, size=R, dtype=np.uint64)
    seeds[0], seeds[1] = 0, 2 ** 64 - 1
    pos = g.integers(0, 2 ** 31 - 1, size=R).astype(np.int32)
    pos[0], pos[2] = 0, 2 ** 31 - 1
    x = torch.randn(R, V, generator=torch.Generator().manual_seed(1)).to(DEV)
    ids, out, u = ops.sample_logits(x, top_p=torch.full((R,), 0.9), seed=sr.seeds_as_int64(seeds), draw_positions=torch.from_numpy(pos),
                                    return_probs=True, return_uniform=True)
    want = sr.philox_uniform(seeds, pos)
    assert np.array_equal(u.cpu().numpy().view(np.uint32), want.view(np.uint32))
    sr.check_rows(x.cpu(), None, None, torch.full((R,), 0.9), torch.from_numpy(want), ids, out)
    mine = torch.rand(R, generator=torch.Generator().manual_seed(2))
    ids2, out2, u2 = ops.sample_logits(x, top_p=torch.full((R,), 0.9), uniform=mine, seed=sr.seeds_as_int64(seeds),
                                       draw_positions=torch.from_numpy(pos), return_probs=True, return_uniform=True)
    assert torch.equal(u2.cpu(), mine) and torch.equal(out2, out)
    sr.check_rows(x.cpu(), None, None, torch.full((R,), 0.9), mine, ids2, out2)


def test_a_row_is_a_pure_function_of_itself():
    """The same row alone, as row 37 of 64 and in a second run: same id, bit-identical probs_out (no dependence on the batch, on the
    row index or on the order in which blocks arrive)."""
    V = 152064
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(64, V, generator=g) * 2.0).to(DEV)
    temp, tk, tp, u = torch.full((64,), 0.7), torch.full((64,), 50, dtype=torch.int32), torch.rand(64, generator=g) * 0.5 + 0.45, torch.rand(64, generator=g)
    tk[37] = 0
    ids, out = ops.sample_logits(x, temp, tk, tp, uniform=u, return_probs=True)
    ids_b, out_b = ops.sample_logits(x, temp, tk, tp, uniform=u, return_probs=True)
    assert torch.equal(ids, ids_b) and torch.equal(out, out_b)
    one = slice(37, 38)
    ids_1, out_1 = ops.sample_logits(x[one].clone(), temp[one], tk[one], tp[one], uniform=u[one], return_probs=True)
    assert int(ids_1[0]) == int(ids[37]) and torch.equal(out_1[0], out[37])
    assert int((out[37] > 0).sum()) > 1000


@pytest.mark.parametrize("B,V,longest", [(3, 97, 7), (5, 4099, 300), (4, 152064, 2500), (2, 1031, 40000)])
def test_apply_penalties_history_matches_oracle(B, V, longest):
    g = torch.Generator().manual_seed(B * 1000 + longest)
    x = torch.randn(B, V, generator=g) * 3
    L = longest + 3                                                      # history_ld: wider than any row's length
    hist = torch.randint(0, min(V, 64 if longest > 1000 else V), (B, L), generator=g, dtype=torch.int32)
    hist[:, ::5] = torch.randint(0, V, (B, (L + 4) // 5), generator=g, dtype=torch.int32)
    hist[0, 1], hist[B - 1, 2], hist[0, 3] = -1, V, V + 7                # ids outside [0, V): skipped
    lens = torch.randint(1, longest + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = longest
    if B > 2:
        lens[1] = 0
    rep, pres, freq = torch.rand(B, generator=g) + 0.6, torch.rand(B, generator=g), torch.rand(B, generator=g) * 0.1
    # the oracle reads output_ids [step][B], skipping nothing: mark what lies past a row's length with -1 (outside the vocabulary)
    ids = hist[:, :longest].clone()
    ids[torch.arange(longest).unsqueeze(0) >= lens.unsqueeze(1)] = -1
    ref = oracle.apply_penalties(x, repetition_penalty=rep, presence_penalty=pres, frequency_penalty=freq,
                                 output_ids=ids.t().contiguous(), max_input_length=0, step=longest)
    got = ops.apply_penalties_history(x.clone().to(DEV), hist.to(DEV), lens.to(DEV), rep, pres, freq).cpu()
    assert torch.equal(got, ref)
    # one penalty alone, and lengths beyond history_ld are clamped to it
    ref1 = oracle.apply_penalties(x, presence_penalty=pres, output_ids=hist[:, :8].t().contiguous(), max_input_length=0, step=8)
    clean = hist[:, :8].contiguous()
    got1 = ops.apply_penalties_history(x.clone().to(DEV), clean.to(DEV), torch.full((B,), 10 ** 6, dtype=torch.int32).to(DEV), presence_penalty=pres).cpu()
    assert torch.equal(got1, ref1)
