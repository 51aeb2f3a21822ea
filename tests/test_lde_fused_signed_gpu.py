"""The fused LDE kernel's forward rounds on signed representatives (bb::dit_signed, ntt::bounds in csrc/ntt.hip): pw_lde_fused against
the oracle's LDE, word for word, and against the unfused schedule (inverse transform, then the coset transform from the coefficients:
pw_lde_batch, the two calls the provers make under POWDR_LDE_FUSED=0) on the same inputs.

Heights: 2^12 (one launch: the conversion to canonical words is the LDE's final store), 2^13 (the smallest height with a strided group
on each side: the forward one takes the kernel's words as its [0, 2p) inputs), 2^16 (three rounds and several tiles per column).
Five columns per height: all p - 1, all 0, alternating 0 / p - 1, one p - 1 at row 0, seeded random."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm

P = om.P
HEIGHTS = [12, 13, 16]
W = 5


def _columns(log_h):
    H = 1 << log_h
    cols = np.zeros((W, H), np.uint32)
    cols[0, :] = P - 1
    cols[2, 1::2] = P - 1
    cols[3, 0] = P - 1
    cols[4] = np.random.default_rng(9500 + log_h).integers(0, P, H, dtype=np.uint32)
    return np.ascontiguousarray(cols).reshape(-1)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from powdr_amd import abi, prover

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    return torch, abi, prover


@pytest.fixture(scope="module")
def oracle_lde():
    """The reference, computed once per height and left unchanged."""
    out = {}
    for log_h in HEIGHTS:
        t = _columns(log_h)
        want = sm.lde(t, W, log_h)
        want.setflags(write=False)
        out[log_h] = (t, want)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("log_h", HEIGHTS)
def test_fused_lde_matches_oracle_and_unfused_schedule(gpu, oracle_lde, monkeypatch, log_h):
    torch, abi, prover = gpu
    monkeypatch.delenv("POWDR_LDE_FUSED_GENERIC", raising=False)
    monkeypatch.delenv("POWDR_NTT_STRIDED_GENERIC", raising=False)
    H = 1 << log_h
    t, want = oracle_lde[log_h]
    d_t = torch.from_numpy(om.to_monty(t).view(np.int32)).cuda()
    d_tmp = torch.empty(W * H, dtype=torch.int32, device="cuda")
    d_fused = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
    d_unfused = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
    abi.check(prover.lib.pw_lde_fused(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), d_fused.data_ptr()), "pw_lde_fused")
    abi.check(prover.lib.pw_lde_batch(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), d_unfused.data_ptr()), "pw_lde_batch")
    torch.cuda.synchronize()
    words = d_fused.cpu().numpy().view(np.uint32)
    assert (words < P).all(), "a stored word is not canonical"
    got = om.from_monty(words).reshape(W, 2 * H)
    ref = np.asarray(want).reshape(W, 2 * H)
    for c, kind in enumerate(["p_minus_1", "zero", "alternating", "p_minus_1_at_row_0", "random"]):
        assert (got[c] == ref[c]).all(), f"{kind}: fused LDE != oracle"
    assert torch.equal(d_fused, d_unfused), "fused LDE != unfused schedule"
