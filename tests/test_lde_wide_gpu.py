"""More columns than one launch takes (blockIdx.y = column, at most 65 535 per launch): every LDE entry point splits a wide matrix
into column chunks. The transforms are linear, so with column c = (c + 1) * column 0 as input, output column c must be (c + 1) *
output column 0 — checked on both sides of the chunk boundary, exactly (field arithmetic), and column 0 against the oracle."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm

P = om.P
W = 65537
CHECKED = [0, 1, 65534, 65535, 65536]
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from powdr_amd import abi, prover

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch, abi, prover


def _words(torch, t):
    """int32 storage -> the unsigned words as int64"""
    return t.to(torch.int64) & 0xFFFFFFFF


def _wide_input(torch, log_h):
    """(canonical column 0 on the host, the W x H matrix of Montgomery words on the device): (c + 1) x R = (c + 1) (x R) mod p"""
    H = 1 << log_h
    col0 = np.random.default_rng(65537 + log_h).integers(0, P, H, dtype=np.uint32)
    m0 = torch.from_numpy(om.to_monty(col0).astype(np.int64)).cuda()
    d = torch.empty(W * H, dtype=torch.int32, device="cuda")
    step = 8192  # columns per product: the 64-bit intermediate stays small
    for c0 in range(0, W, step):
        c1 = min(W, c0 + step)
        k = torch.arange(c0 + 1, c1 + 1, dtype=torch.int64, device="cuda")
        d[c0 * H:c1 * H] = ((k[:, None] * m0[None, :]) % P).to(torch.int32).reshape(-1)
    return col0, d


def _assert_multiples_of_column_0(torch, d_out, n, what):
    """d_out: W columns of n words; column c = (c + 1) * column 0 mod p for the checked columns, in 64-bit integers on the device"""
    out = d_out.view(W, n)
    c0 = _words(torch, out[0]) % P
    for c in CHECKED:
        got = _words(torch, out[c]) % P
        assert torch.equal(got, ((c + 1) * c0) % P), f"{what}: column {c} != {c + 1} * column 0"


def _from_dev(t):
    return om.from_monty(t.cpu().numpy().view(np.uint32))


def test_four_pass_schedule(gpu):
    torch, abi, prover = gpu
    log_h = 2
    H = 1 << log_h
    col0, d_t = _wide_input(torch, log_h)
    d_c = torch.empty(W * H, dtype=torch.int32, device="cuda")
    d_l = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
    abi.check(prover.lib.pw_lde_batch(d_t.data_ptr(), W, log_h, d_c.data_ptr(), d_l.data_ptr()), "pw_lde_batch")
    torch.cuda.synchronize()
    _assert_multiples_of_column_0(torch, d_l, 2 * H, "pw_lde_batch")
    assert (_from_dev(d_l[:2 * H]) == sm.lde(col0, 1, log_h)).all(), "column 0 != oracle"


@pytest.mark.parametrize("log_h", [2, 12, 13])
def test_fused_schedule(gpu, monkeypatch, log_h):
    """2^2 rows: the generic fused kernel; 2^12: the specialised kernel alone; 2^13: strided groups on both sides of it."""
    torch, abi, prover = gpu
    monkeypatch.delenv("POWDR_LDE_FUSED_GENERIC", raising=False)
    H = 1 << log_h
    col0, d_t = _wide_input(torch, log_h)
    d_tmp = torch.empty(W * H, dtype=torch.int32, device="cuda")
    d_l = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
    abi.check(prover.lib.pw_lde_fused(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), d_l.data_ptr()), "pw_lde_fused")
    torch.cuda.synchronize()
    _assert_multiples_of_column_0(torch, d_l, 2 * H, "pw_lde_fused")
    assert (_from_dev(d_l[:2 * H]) == sm.lde(col0, 1, log_h)).all(), "column 0 != oracle"
    del d_t, d_tmp, d_l
    torch.cuda.empty_cache()


def test_subcoset_and_back_to_the_trace(gpu):
    torch, abi, prover = gpu
    log_h, log_blocks = 3, 1
    H = 1 << log_h
    B = 1 << log_blocks
    m = 2 * H // B
    col0, d_t = _wide_input(torch, log_h)
    want = sm.lde(col0, 1, log_h)
    d_c = torch.empty(W * H, dtype=torch.int32, device="cuda")
    d_l = torch.empty(W * 2 * H, dtype=torch.int32, device="cuda")
    abi.check(prover.lib.pw_lde_batch(d_t.data_ptr(), W, log_h, d_c.data_ptr(), d_l.data_ptr()), "pw_lde_batch")
    d_s = torch.empty(1 << 13, dtype=torch.int32, device="cuda")
    d_o = torch.empty(W * m, dtype=torch.int32, device="cuda")
    for r in range(B):
        d_o.zero_()
        abi.check(prover.lib.pw_lde_subcoset(d_c.data_ptr(), W, log_h, log_blocks, r, d_s.data_ptr(), d_o.data_ptr()), "pw_lde_subcoset")
        torch.cuda.synchronize()
        _assert_multiples_of_column_0(torch, d_o, m, f"pw_lde_subcoset r = {r}")
        assert (_from_dev(d_o[:m]) == want[r::B]).all(), f"sub-coset {r}: column 0 != oracle"
    abi.check(prover.lib.pw_trace_from_coefficients(d_c.data_ptr(), W, log_h, d_s.data_ptr()), "pw_trace_from_coefficients")
    torch.cuda.synchronize()
    assert torch.equal(d_c, d_t), "pw_trace_from_coefficients did not give back the input"
