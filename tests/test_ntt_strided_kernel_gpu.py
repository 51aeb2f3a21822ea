"""The strided stage groups of the fused LDE schedule at 2^20 rows (ntt_strided_kernel<DIF, 8>, fixed geometry) against the generic
ntt_group_kernel (POWDR_NTT_STRIDED_GENERIC=1, read per call), the four-pass schedule (pw_lde_batch, which never reaches the new
kernel) and the oracle: word for word (exact field arithmetic). `powdr_gpu_call_stats` says which kernel ran."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm

P = om.P
KINDS = ["random", "zero", "p_minus_1", "one_at_row_0", "one_at_last_row"]
FIXED_HEIGHTS = [20]  # the heights with a fixed-geometry instantiation (K = log_h - 12)
STAT = "ntt_strided_fixed_launches"


@pytest.fixture(scope="module")
def gpu():
    import torch
    from powdr_amd import abi, prover

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    return torch, abi, prover


def _input(kind, W, H, seed):
    """Canonical words, column-major W x H; the edge kinds repeat one column W times."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, P, W * H, dtype=np.uint32)
    col = np.zeros(H, np.uint32)
    if kind == "p_minus_1":
        col[:] = P - 1
    elif kind == "one_at_row_0":
        col[0] = 1
    elif kind == "one_at_last_row":
        col[H - 1] = 1
    return np.tile(col, W)


def _three_ldes(torch, abi, prover, monkeypatch, t, W, log_h):
    """(fused schedule, fused schedule with the generic strided kernel, four-pass schedule), and the counter after each."""
    H = 1 << log_h
    d_t = torch.from_numpy(om.to_monty(t).view(np.int32)).cuda()
    d_tmp = torch.empty(W * H, dtype=torch.int32, device="cuda")
    outs = [torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda") for _ in range(3)]
    counts = []
    monkeypatch.delenv("POWDR_NTT_STRIDED_GENERIC", raising=False)
    abi.call_stats(reset=True)
    abi.check(prover.lib.pw_lde_fused(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), outs[0].data_ptr()), "pw_lde_fused")
    counts.append(abi.call_stats(reset=True)[STAT])
    monkeypatch.setenv("POWDR_NTT_STRIDED_GENERIC", "1")
    abi.check(prover.lib.pw_lde_fused(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), outs[1].data_ptr()), "pw_lde_fused (generic strided)")
    counts.append(abi.call_stats(reset=True)[STAT])
    monkeypatch.delenv("POWDR_NTT_STRIDED_GENERIC")
    abi.check(prover.lib.pw_lde_batch(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), outs[2].data_ptr()), "pw_lde_batch")
    counts.append(abi.call_stats(reset=True)[STAT])
    torch.cuda.synchronize()
    return outs, counts


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("log_h", FIXED_HEIGHTS)
def test_fixed_kernel_matches_generic_four_pass_and_oracle(gpu, monkeypatch, log_h, W):
    torch, abi, prover = gpu
    H = 1 << log_h
    for kind in KINDS:
        t = _input(kind, W, H, seed=1000 * log_h + W)
        (d_fixed, d_gen, d_four), counts = _three_ldes(torch, abi, prover, monkeypatch, t, W, log_h)
        # one launch per direction (both groups of the schedule), none in the other two calls
        assert counts == [2, 0, 0], f"{kind}: launches of the fixed-geometry kernel per call {counts}"
        assert torch.equal(d_fixed, d_gen), f"{kind}: fixed-geometry != generic strided kernel"
        assert torch.equal(d_fixed, d_four), f"{kind}: fixed-geometry != four-pass schedule"
        if kind == "random" and W == 1:
            got = om.from_monty(d_fixed.cpu().numpy().view(np.uint32))
            assert (got == sm.lde(t, 1, log_h)).all(), "!= oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 3])
def test_other_geometry_keeps_the_generic_kernel(gpu, monkeypatch, W):
    """2^17 rows: 64-byte segments (c = 4), not the fixed kernel's geometry — the counter stays 0 and the words still agree."""
    torch, abi, prover = gpu
    log_h = 17
    for kind in KINDS:
        t = _input(kind, W, 1 << log_h, seed=1000 * log_h + W)
        (d_fixed, d_gen, d_four), counts = _three_ldes(torch, abi, prover, monkeypatch, t, W, log_h)
        assert counts == [0, 0, 0], f"{kind}: launches of the fixed-geometry kernel per call {counts}"
        assert torch.equal(d_fixed, d_gen) and torch.equal(d_fixed, d_four), kind


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [False, True])
def test_whole_proof_at_2_20_rows(gpu, monkeypatch, generic):
    """One proof of 2 columns x 2^20 rows, one degree-2 constraint, no LogUp: the words are the oracle's with either strided kernel."""
    from tests.test_prover_gpu import _prove_both_and_compare

    torch, abi, prover = gpu
    if generic:
        monkeypatch.setenv("POWDR_NTT_STRIDED_GENERIC", "1")
    else:
        monkeypatch.delenv("POWDR_NTT_STRIDED_GENERIC", raising=False)
    W, log_h = 2, 20
    flat = np.random.default_rng(20).integers(0, P, W << log_h, dtype=np.uint32)
    bc = np.array([om.OP_PUSH_APC, 0, om.OP_PUSH_APC, 1, om.OP_MUL], np.uint32)
    spans = np.array([[0, len(bc)]], np.uint32)
    abi.call_stats(reset=True)
    _prove_both_and_compare(torch, prover, flat, W, log_h, bc, spans, None, nq=5, pow_bits=0, satisfied=False)
    assert (abi.call_stats()[STAT] > 0) == (not generic)
