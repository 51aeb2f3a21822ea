"""The fused LDE kernel specialised for 2^12 rows and more against the generic fused kernel (POWDR_LDE_FUSED_GENERIC=1, read per
call), the four-pass schedule (pw_lde_batch) and, up to 2^16 rows, the oracle: word for word (exact field arithmetic)."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm

P = om.P
KINDS = ["random", "zero", "p_minus_1", "one_at_row_0", "one_at_last_row"]


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


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 2, 7, 300])
@pytest.mark.parametrize("log_h", list(range(12, 21)))
def test_specialised_kernel_matches_generic_four_pass_and_oracle(gpu, monkeypatch, log_h, W):
    torch, abi, prover = gpu
    H = 1 << log_h
    for kind in KINDS:
        t = _input(kind, W, H, seed=1000 * log_h + W)
        d_t = torch.from_numpy(om.to_monty(t).view(np.int32)).cuda()
        d_tmp = torch.empty(W * H, dtype=torch.int32, device="cuda")
        d_spec = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
        d_gen = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
        d_four = torch.zeros(W * 2 * H, dtype=torch.int32, device="cuda")
        monkeypatch.delenv("POWDR_LDE_FUSED_GENERIC", raising=False)
        abi.check(prover.lib.pw_lde_fused(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), d_spec.data_ptr()), "pw_lde_fused")
        monkeypatch.setenv("POWDR_LDE_FUSED_GENERIC", "1")
        abi.check(prover.lib.pw_lde_fused(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), d_gen.data_ptr()), "pw_lde_fused (generic)")
        monkeypatch.delenv("POWDR_LDE_FUSED_GENERIC")
        abi.check(prover.lib.pw_lde_batch(d_t.data_ptr(), W, log_h, d_tmp.data_ptr(), d_four.data_ptr()), "pw_lde_batch")
        torch.cuda.synchronize()
        assert torch.equal(d_spec, d_gen), f"{kind}: specialised != generic fused kernel"
        assert torch.equal(d_spec, d_four), f"{kind}: specialised != four-pass schedule"
        if log_h <= 16:
            got = om.from_monty(d_spec.cpu().numpy().view(np.uint32))
            if kind == "random":
                assert (got == sm.lde(t, W, log_h)).all(), f"{kind}: != oracle"
            else:  # W copies of one column
                want = sm.lde(t[:H], 1, log_h)
                assert (got.reshape(W, 2 * H) == want[None, :]).all(), f"{kind}: != oracle"
        del d_t, d_tmp, d_spec, d_gen, d_four


@pytest.mark.gpu
def test_whole_proof_through_small_panels_at_2_14_rows(gpu, monkeypatch):
    """Panels of 8 columns (many small launches, blockIdx.y > 0) with the fused schedule forced at 2^14 rows (the provers' own
    rule takes the four-pass one there): the proof words are the oracle's."""
    from tests.test_prover_gpu import _prove_both_and_compare

    torch, abi, prover = gpu
    monkeypatch.setenv("POWDR_PANEL_LOG_WORDS", "12")
    monkeypatch.setenv("POWDR_LDE_FUSED", "1")
    W, log_h = 45, 14
    rng = np.random.default_rng(14)
    flat = rng.integers(0, P, W << log_h, dtype=np.uint32)
    PA, PC = om.OP_PUSH_APC, om.OP_PUSH_CONST
    bc, spans = [], []
    for _ in range(5):
        off = len(bc)
        a, b, c = (int(x) for x in rng.integers(0, W, 3))
        bc += [PA, a, PA, b, om.OP_MUL, PA, c, om.OP_MUL, PC, int(rng.integers(0, P)), om.OP_ADD]
        spans.append((off, len(bc) - off))
    bc, spans = np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2)
    _prove_both_and_compare(torch, prover, flat, W, log_h, bc, spans, None, nq=5, pow_bits=0, satisfied=False)
