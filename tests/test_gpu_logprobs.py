"""mi355_logprobs on the GPU against the float64 reference of tests/logprob_ref.py: token value, log-sum-exp and top-N records, with
sentinels behind every output array.

Inputs: a background of normal values clipped to <= 2.0 plus N + 1 head entries at random indices (one at index 0, one in the last,
partial segment) valued 3.0 + 0.05 i: after any temperature in [0.5, 2] the top N + 1 scaled values differ by at least 0.025, far
above MIN_GAP, which is asserted on the reference before the reported ids are required to equal the reference's exactly."""
import numpy as np
import pytest
import torch

from rtp_llm_amd import _C, ops
from tests import logprob_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT, ISENT, GUARD = -12345.5, -777, 64
NEG = float("-inf")


def seg_len(V):
    return (((V + 31) // 32) + 3) & ~3


def make_rows(R, V, n_head, seed, neg_frac=0.0):
    """-> (logits [R, V] fp32 on the host, head indices [R][...])."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g).clamp_(max=2.0)
    if neg_frac:
        x[torch.rand(R, V, generator=g) < neg_frac] = NEG
    heads = []
    last_lo = ((V - 1) // seg_len(V)) * seg_len(V)             # first index of the last segment that holds anything
    for r in range(R):
        k = min(n_head, V)
        idx = [0]
        if k > 1:
            idx.append(int(torch.randint(max(last_lo, 1), V, (1,), generator=g)))
        perm = torch.randperm(V, generator=g).tolist()
        for j in perm:
            if len(idx) >= k:
                break
            if j not in idx:
                idx.append(j)
        order = torch.randperm(k, generator=g).tolist()        # which head entry gets which value
        for i, j in zip(order, idx):
            x[r, j] = 3.0 + 0.05 * i
        heads.append(idx)
    return x, heads


def run_op(x, temperature=None, ids=None, top_n=0, top_ld=None):
    """The raw entry point on x [R, V] (a device tensor, possibly a strided view) with guarded outputs; the guards and the spare
    columns of the top arrays are checked here."""
    R, V = x.shape
    ld = x.stride(0) if R > 1 else max(V, x.stride(0))
    top_ld = top_n if top_ld is None else top_ld
    f = lambda n: torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
    tok, lse, tlp = f(R), f(R), f(R * top_ld)
    tid = torch.full((R * top_ld + GUARD,), ISENT, dtype=torch.int32, device=DEV)
    temp = None if temperature is None else torch.as_tensor(temperature, dtype=torch.float32).to(DEV)
    idt = None if ids is None else torch.as_tensor(ids, dtype=torch.int32).to(DEV)
    l = _C.lib()
    nbytes = l.mi355_logprobs_workspace_bytes(R, V, top_n)
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    ws[nbytes:] = 0x5A
    p = lambda t: None if t is None else t.data_ptr()
    _C.check(l.mi355_logprobs(x.data_ptr(), R, V, ld, p(temp), p(idt), top_n, p(tok) if ids is not None else None, lse.data_ptr(),
                              p(tid) if top_n else None, p(tlp) if top_n else None, top_ld, ws.data_ptr(), nbytes,
                              torch.cuda.current_stream().cuda_stream), "logprobs")
    torch.cuda.synchronize()
    assert (tok[R:] == SENT).all() and (lse[R:] == SENT).all() and (tlp[R * top_ld:] == SENT).all() and (tid[R * top_ld:] == ISENT).all()
    assert (ws[nbytes:] == 0x5A).all()
    if ids is None:
        assert (tok == SENT).all()
    tid2, tlp2 = tid[: R * top_ld].view(R, top_ld), tlp[: R * top_ld].view(R, top_ld)
    assert (tid2[:, top_n:] == ISENT).all() and (tlp2[:, top_n:] == SENT).all()
    return {"token": tok[:R].cpu(), "lse": lse[:R].cpu(), "top_ids": tid2[:, :top_n].cpu(), "top_lp": tlp2[:, :top_n].cpu()}


def bits(t):
    return t.reshape(-1).view(torch.int32).tolist()


def check(res, x_host, temperature, ids, top_n, ties=False):
    ref = lr.reference(x_host, temperature, ids, top_n)
    lr.assert_close(res["lse"], ref["lse"], "lse")
    if ids is not None:
        lr.assert_close(res["token"], ref["token"], "token value")
    if top_n:
        if not ties:
            assert (ref["gap"] >= lr.MIN_GAP).all(), "the inputs do not separate the reference's top N + 1 values"
        assert np.array_equal(res["top_ids"].numpy(), ref["top_ids"]), "top ids"
        lr.assert_close(res["top_lp"], ref["top_lp"], "top values")
        # a listed value and the token value of the same index are the same fp32 number
        if ids is not None:
            for r in range(x_host.shape[0]):
                hit = (res["top_ids"][r] == int(ids[r])).nonzero()
                if len(hit):
                    assert bits(res["top_lp"][r, int(hit[0])]) == bits(res["token"][r])
    return ref


def dev_view(x_host, ld=None, offset=0):
    """x on the device as rows of a wider buffer (ld) starting `offset` floats into it; the padding holds large values that must
    never be read into a result."""
    R, V = x_host.shape
    ld = V if ld is None else ld
    buf = torch.full((R * ld + offset + 8,), 1e30, dtype=torch.float32, device=DEV)
    v = buf[offset: offset + R * ld].view(R, ld)[:, :V]
    v.copy_(x_host)
    return v


SHAPES = [  # rows, V, ld, top_n
    (1, 5, 5, 8),                 # V < N, empty segments
    (3, 1003, 1003, 20),          # scalar path
    (3, 1003, 1008, 20),          # vector path, padding never read into a result
    (64, 4099, 4099, 20),         # many rows, partial last segment
    (2, 152064, 152064, 20),      # full sum length
    (1, 200003, 200004, 5),       # a segment longer than one staged chunk
]


@pytest.mark.parametrize("R,V,ld,n", SHAPES)
@pytest.mark.parametrize("with_temp", [False, True])
def test_values_and_ids_against_the_reference(R, V, ld, n, with_temp):
    x, heads = make_rows(R, V, n + 1, seed=V + R)
    g = torch.Generator().manual_seed(9)
    temp = (0.5 + 1.5 * torch.rand(R, generator=g)) if with_temp else None
    ids = torch.randint(0, V, (R,), generator=g)
    ids[0] = heads[0][0]                                       # a head entry: also listed
    res = run_op(dev_view(x, ld), temp, ids, n)
    ref = check(res, x, temp, ids, n)
    if V < n:
        assert (res["top_ids"][:, V:] == -1).all() and (res["top_lp"][:, V:] == NEG).all()
    assert int(ids[0]) in ref["top_ids"][0]


@pytest.mark.parametrize("R,V,ld,n", [(3, 1003, 1008, 20), (64, 4099, 4099, 20)])
def test_minus_infinity_and_nan_entries(R, V, ld, n):
    x, heads = make_rows(R, V, n + 1, seed=77 + V, neg_frac=0.10)
    ids = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(3))
    dead = [int(((x[r] == NEG).nonzero())[0]) for r in range(R)]
    ids[0] = dead[0]                                           # a chosen id on a -inf entry
    bg = [j for j in range(V) if j not in heads[1] and x[1, j] > NEG][:2]
    x[1, bg[0]] = float("nan"); ids[1] = bg[0]                 # a NaN entry counts as -inf: skipped, and -inf as a token value
    x[2, heads[2][3]] = float("nan")                           # a NaN where a head entry was: never listed
    temp = torch.tensor([0.8] * R)
    res = run_op(dev_view(x, ld), temp, ids, n)
    check(res, x, temp, ids, n)
    assert res["token"][0] == NEG and res["token"][1] == NEG
    assert heads[2][3] not in res["top_ids"][2].tolist() and torch.isfinite(res["lse"]).all()
    # a row with fewer live entries than top_n: padded
    y = torch.full((1, 1003), NEG); y[0, [5, 700, 64]] = torch.tensor([1.0, 1.0, 2.0])
    r2 = run_op(dev_view(y, 1003), None, [5], 8)
    check(r2, y, None, torch.tensor([5]), 8, ties=True)
    assert r2["top_ids"][0].tolist() == [64, 5, 700, -1, -1, -1, -1, -1]


def test_one_dominant_entry():
    x, _ = make_rows(3, 4099, 9, seed=21)
    x[0, 4098] += 60.0; x[1, 0] += 60.0; x[2, 2000] += 60.0
    ids = torch.tensor([4098, 17, 2000])
    for temp in (None, torch.tensor([1.0, 0.5, 2.0])):
        res = run_op(dev_view(x), temp, ids, 8)
        check(res, x, temp, ids, 8)
        assert abs(float(res["token"][0])) < 1e-5 and float(res["token"][1]) < -50.0


def test_exact_ties_keep_index_order():
    """temperature NULL: runs of equal values across a segment boundary and across the top-N boundary, lower index first."""
    V, n = 1003, 6
    assert seg_len(V) == 32
    x = torch.randn(3, V, generator=torch.Generator().manual_seed(4)).clamp_(max=2.0)
    x[0, 60:70] = 5.0                                          # boundary of segments 1 | 2 at 64; the run is cut by N
    x[1, 60:70] = 5.0; x[1, 500] = 6.0; x[1, 3] = 5.5
    x[2, 10::30] = 5.0                                         # one equal per segment or so
    res = run_op(dev_view(x), None, [60, 63, 40], n)
    check(res, x, None, torch.tensor([60, 63, 40]), n, ties=True)
    assert res["top_ids"][0].tolist() == [60, 61, 62, 63, 64, 65]
    assert res["top_ids"][1].tolist() == [500, 3, 60, 61, 62, 63]
    assert res["top_ids"][2].tolist() == [10, 40, 70, 100, 130, 160]
    # full width: a run over a segment boundary with many equals per lane and wave, a row of equal values, and -0 == +0
    V, n = 152064, 32
    s = seg_len(V)
    y = torch.randn(3, V, generator=torch.Generator().manual_seed(6)).clamp_(max=2.0)
    y[0, s - 252: s + 348] = 4.0
    y[1, :] = 1.0
    y[2] = y[2].clamp(max=-1.0); y[2, 7] = 0.0; y[2, 5] = -0.0; y[2, 90000] = 0.0
    res = run_op(dev_view(y), None, [s, 9, 5], n)
    check(res, y, None, torch.tensor([s, 9, 5]), n, ties=True)
    assert res["top_ids"][0].tolist() == list(range(s - 252, s - 252 + n))
    assert res["top_ids"][1].tolist() == list(range(n))
    assert res["top_ids"][2, :3].tolist() == [5, 7, 90000]
    assert bits(res["top_lp"][2, 0]) == bits(res["top_lp"][2, 1]) == bits(res["token"][2])


@pytest.mark.parametrize("n", [0, 1, 32])
def test_top_n_range_and_spare_columns(n):
    x, _ = make_rows(3, 1003, 33, seed=31)
    temp, ids = torch.tensor([0.5, 1.0, 2.0]), torch.tensor([0, 500, 1002])
    res = run_op(dev_view(x, 1008), temp, ids, n, top_ld=n + 3)           # spare columns keep their sentinel (checked in run_op)
    check(res, x, temp, ids, n)
    only = run_op(dev_view(x, 1008), temp, None, n)                        # no ids: token_logprobs untouched
    assert torch.equal(only["lse"].view(torch.int32), res["lse"].view(torch.int32))


def test_strided_views_and_ids_outside_the_row():
    x, _ = make_rows(3, 1003, 9, seed=41)
    ids = torch.tensor([1003, -1, 4])
    ref = None
    for ld, off in ((1003, 0), (1027, 0), (1028, 0), (1028, 1), (1003, 3)):    # scalar and vector paths, misaligned bases
        res = run_op(dev_view(x, ld, off), None, ids, 8)
        check(res, x, None, ids, 8)
        assert torch.isnan(res["token"][:2]).all() and torch.isfinite(res["token"][2])
        if ref is not None:                                    # the outputs do not depend on ld or on the load path
            for k in res:
                assert torch.equal(res[k].view(torch.int32), ref[k].view(torch.int32)), (k, ld, off)
        ref = res
    # the public wrapper takes a strided view as well
    v = dev_view(x, 1028)
    w = ops.logprobs(v, ids=torch.tensor([0, 1, 4]), top_n=8)
    assert torch.equal(w["top_ids"].cpu(), ref["top_ids"]) and torch.equal(w["lse"].cpu(), ref["lse"])
    assert float(w["token_logprobs"][2]) == float(ref["token"][2])


def test_a_row_does_not_depend_on_the_batch_or_the_call():
    x, _ = make_rows(64, 4099, 21, seed=51)
    g = torch.Generator().manual_seed(8)
    temp = 0.5 + 1.5 * torch.rand(64, generator=g)
    ids = torch.randint(0, 4099, (64,), generator=g)
    full = run_op(dev_view(x), temp, ids, 20)
    again = run_op(dev_view(x), temp, ids, 20)
    alone = run_op(dev_view(x[63:64]), temp[63:], ids[63:], 20)
    first = run_op(dev_view(x[63:64].repeat(2, 1), 4100), temp[63:].repeat(2), ids[63:].repeat(2), 20)   # as rows 0 and 1, vector path
    for k in full:
        a = full[k].view(torch.int32)
        assert torch.equal(a, again[k].view(torch.int32)), k
        assert torch.equal(a[63:64], alone[k].view(torch.int32)), k
        assert torch.equal(a[63:64], first[k].view(torch.int32)[:1]) and torch.equal(a[63:64], first[k].view(torch.int32)[1:]), k
