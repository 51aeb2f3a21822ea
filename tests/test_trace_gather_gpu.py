"""pw_trace_gather_rows on the GPU: the gather kernel alone, on outputs pre-filled with 0xA5A5A5A5, compared word for
word with numpy indexing. Every shape of a kind travels as one job of ONE call, so every call here is also a many-job launch."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ZERO_ROW = 0xFFFFFFFF
FILL = 0xA5A5A5A5
TILE = 1024       # output rows of a workgroup
COL_GROUP = 16    # columns of a workgroup
H_OUTS = (1, 2, 4, 8, 1024, 2048, 4096)
COUNTS = (0, 1, 3, 4, 5, TILE - 1, TILE, TILE + 1)
WIDTHS = (1, 3, COL_GROUP + 1)
H_INS = (2, 4, 1 << 12)


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import apc_sources

    return torch, apc_sources


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).cuda()


def expected(src, idx):
    """src [width, h_in], idx [h_out] -> [width, h_out]"""
    h_in = src.shape[1]
    return np.where(idx[None, :] < h_in, src[:, np.minimum(idx, h_in - 1)], 0).astype(np.uint32)


def run(gpu, cases, shift_out=0):
    """cases: [(src [width, h_in], idx [h_out])] as the jobs of one call -> the outputs [width, h_out]; shift_out: words the outputs start
    past a 16-byte boundary"""
    torch, aps = gpu
    keep, jobs, outs = {}, [], []
    for src, idx in cases:
        if id(src) not in keep:
            keep[id(src)] = to_dev(torch, src)
        d_idx = to_dev(torch, idx)
        d_out = torch.full((src.shape[0] * len(idx) + shift_out,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
        outs.append((d_out, d_idx))
        jobs.append(aps.GatherJob(keep[id(src)].data_ptr(), src.shape[1], src.shape[0], d_idx.data_ptr(), d_out.data_ptr() + 4 * shift_out, len(idx)))
    torch.cuda.synchronize()
    aps.gather_rows(jobs)
    got = []
    for (d_out, _), (src, idx) in zip(outs, cases):
        words = d_out.cpu().numpy().view(np.uint32)
        assert (words[:shift_out] == FILL).all()
        got.append(words[shift_out:].reshape(src.shape[0], len(idx)))
    return got


def check(gpu, cases, **kw):
    for k, (got, (src, idx)) in enumerate(zip(run(gpu, cases, **kw), cases)):
        want = expected(src, idx)
        assert (got == want).all(), (k, src.shape, len(idx), np.argwhere(got != want)[:4].tolist())


@pytest.fixture(scope="module")
def sources():
    rng = np.random.default_rng(0x6a7)
    return {(w, h): rng.integers(1, 1 << 32, size=(w, h), dtype=np.uint64).astype(np.uint32) for w in WIDTHS for h in H_INS}


def index_list(kind, n, h_out, h_in, rng):
    """the first n entries name rows by `kind`, the tail is zero rows"""
    i = np.arange(h_out, dtype=np.int64)
    if kind.startswith("run"):  # a run starting at a residue mod 4 (run0: the identity)
        idx = (i + int(kind[3:])) % h_in
    elif kind == "holes":  # runs of 3 with holes: 0 1 2 . 4 5 6 . 8 ...
        idx = (i + i // 3) % h_in
    elif kind == "permutation":
        idx = np.concatenate([rng.permutation(h_in) for _ in range(h_out // h_in + 1)])[:h_out]
    elif kind == "zero_inside":  # a zero row in the middle of a lane's four
        idx = np.where(i % 4 == 1 + (i // 4) % 2, ZERO_ROW, i % h_in)
    elif kind == "same4":  # the same source row four times
        idx = (i // 4) % h_in
    else:
        assert kind == "all_zero"
        idx = np.full(h_out, ZERO_ROW, np.int64)
    idx = idx.astype(np.uint32)
    idx[n:] = ZERO_ROW
    return idx


KINDS = ("run0", "run1", "run2", "run3", "holes", "permutation", "all_zero", "zero_inside", "same4")


@pytest.mark.parametrize("kind", KINDS)
def test_every_shape_of_an_index_list(gpu, sources, kind):
    rng = np.random.default_rng([KINDS.index(kind), 5])
    cases = []
    for h_out, n, w, h_in in itertools.product(H_OUTS, COUNTS, WIDTHS, H_INS):
        if n > h_out:
            continue
        cases.append((sources[(w, h_in)], index_list(kind, n, h_out, h_in, rng)))
    assert len(cases) > 300
    check(gpu, cases)
    stats = gpu[1].last_stats()
    assert stats["gather_jobs"] == len(cases) and stats["scratch_bytes"] == 0
    # a tile is 1 024 rows x 16 columns: every job's tiles are counted once
    tiles = sum(-(-len(idx) // TILE) * -(-src.shape[0] // COL_GROUP) for src, idx in cases)
    assert stats["tiles_16_byte_loads"] + stats["tiles_4_byte_loads"] == tiles


def test_both_load_paths_are_taken(gpu, sources):
    aps = gpu[1]
    src = sources[(3, 1 << 12)]
    rng = np.random.default_rng(9)
    check(gpu, [(src, np.arange(4096, dtype=np.uint32))])
    stats = aps.last_stats()
    assert stats["tiles_16_byte_loads"] == 4 and stats["tiles_4_byte_loads"] == 0
    check(gpu, [(src, rng.permutation(4096).astype(np.uint32))])
    stats = aps.last_stats()
    assert stats["tiles_16_byte_loads"] == 0 and stats["tiles_4_byte_loads"] == 4
    # runs with holes where calls were: one tile of each kind in one call
    idx = np.arange(4096, dtype=np.uint32)
    idx[1024:2048] = np.sort(rng.permutation(4096)[:1024]).astype(np.uint32)
    check(gpu, [(src, idx)])
    stats = aps.last_stats()
    assert stats["tiles_16_byte_loads"] == 3 and stats["tiles_4_byte_loads"] == 1 and stats["gather_jobs"] == 1
    # all zero rows: no load at all
    check(gpu, [(src, np.full(2048, ZERO_ROW, np.uint32))])
    assert aps.last_stats()["tiles_4_byte_loads"] == 0


def test_two_jobs_of_different_widths_and_heights(gpu, sources):
    rng = np.random.default_rng(11)
    check(gpu, [(sources[(3, 4)], rng.integers(0, 4, size=2048).astype(np.uint32)), (sources[(17, 1 << 12)], np.arange(1024, dtype=np.uint32)[::-1].copy()),
                (sources[(1, 2)], np.array([1, ZERO_ROW], np.uint32))])


def test_forty_jobs_of_one_tile_each(gpu, sources):
    rng = np.random.default_rng(12)
    cases = []
    for k in range(40):
        idx = (np.arange(1024) + 4 * k).astype(np.uint32) if k % 2 else rng.integers(0, 1 << 12, size=1024).astype(np.uint32)
        cases.append((sources[((1, 3, 1)[k % 3], 1 << 12)], idx))
    check(gpu, cases)
    stats = gpu[1].last_stats()
    assert stats["gather_jobs"] == 40 and stats["tiles_16_byte_loads"] == 20 and stats["tiles_4_byte_loads"] == 20


def test_an_index_that_is_no_row_and_outputs_off_the_16_byte_grid(gpu, sources):
    rng = np.random.default_rng(13)
    idx = rng.integers(0, 8, size=2048).astype(np.uint32)  # rows 4 .. 7 do not exist: zero rows
    check(gpu, [(sources[(3, 4)], idx)])
    for shift in (1, 2, 3):  # an output that is not 16-byte aligned goes word by word
        check(gpu, [(sources[(17, 1 << 12)], np.arange(2048, dtype=np.uint32)), (sources[(3, 4)], idx)], shift_out=shift)
        assert gpu[1].last_stats()["tiles_16_byte_loads"] == 0


def test_an_output_beyond_2_to_the_32_bytes(gpu):
    """2^24 rows x 65 columns: the last column starts at element 2^30, byte 2^32, of its matrix"""
    torch, aps = gpu
    h_out, w, h_in = 1 << 24, 65, 1 << 12
    free, _ = torch.cuda.mem_get_info()
    if free < 7 << 30:
        pytest.skip(f"needs 7 GB of free device memory, {free >> 30} GB are free")
    g = torch.Generator(device="cuda").manual_seed(14)
    src = torch.randint(-(1 << 31), (1 << 31) - 1, (w, h_in), dtype=torch.int32, device="cuda", generator=g)
    i = torch.arange(h_out, dtype=torch.int64, device="cuda")
    idx = torch.where(i < h_out // 2, i % h_in, i * 5 % h_in)  # the first half is runs, the second never has two consecutive rows
    idx[(i % 64) // 4 == 1] = ZERO_ROW                         # whole lanes of zero rows
    d_idx = torch.where(idx > 0x7FFFFFFF, idx - (1 << 32), idx).to(torch.int32)
    out = torch.full((w * h_out,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    aps.gather_rows([aps.GatherJob(src.data_ptr(), h_in, w, d_idx.data_ptr(), out.data_ptr(), h_out)])
    zero = idx == ZERO_ROW
    safe = torch.where(zero, torch.zeros_like(idx), idx)
    for c in (0, 1, 31, 63, 64):
        want = torch.where(zero, torch.zeros((), dtype=torch.int32, device="cuda"), src[c][safe])
        assert torch.equal(out[c * h_out:(c + 1) * h_out], want), c
    stats = aps.last_stats()
    assert stats["tiles_16_byte_loads"] + stats["tiles_4_byte_loads"] == (h_out // TILE) * 5 and stats["tiles_16_byte_loads"] > 0 and stats["tiles_4_byte_loads"] > 0


def test_every_refusal(gpu):
    torch, aps = gpu
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = t.data_ptr()
    good = dict(src=p, h_in=4, width=2, idx=p, out=p + 128, h_out=4)
    bad = [dict(src=None), dict(idx=None), dict(out=None), dict(h_in=3), dict(h_in=0), dict(h_out=6), dict(h_out=0), dict(width=0), dict(h_in=1 << 32)]
    for change in bad:
        with pytest.raises(ValueError, match="malformed"):
            aps.gather_rows([aps.GatherJob(**good), aps.GatherJob(**{**good, **change})])
    assert aps.lib.pw_trace_gather_rows(None, 3) == -1
    aps.gather_rows([])
    assert (t.cpu().numpy() == 0).all()
