"""The Python side of the trace pipelines' entry contract (powdr_amd/stage.py), without a GPU: the messages of the six
stage errors pinned to the strings their separate classes produced before they shared a base, the handle's life cycle, the layout
of the AIR records, the one meaning of the return code -1, and the call-list check the two entries that take calls share."""
import ctypes as C
import gc
import importlib

import pytest

# (class, keyword arguments, status, info, str(error)): every (class, status) pair with a decoding and the undecoded status 6. The
# strings were produced by the classes as they stood before stage.py, with the info values of test_the_error_decodes_its_info, a
# witness pack_witness(3, 5, 9), register 7, call 4, position 6 (status 12) and position 2 (statuses 13, 14).
MESSAGES = [
    ("empirical.EmpiricalError", {}, 2, 0x1000, 'pw_empirical_detect: status 2, the scratch bound is too small (4096 bytes needed)'),
    ("empirical.EmpiricalError", {}, 3, 0x200000009, 'pw_empirical_detect: status 3, not block-structured (head at segment 2, timestamp 9)'),
    ("empirical.EmpiricalError", {}, 4, 0x200000009, 'pw_empirical_detect: status 4, two rows with one time key (segment 2, timestamp 9)'),
    ("empirical.EmpiricalError", {}, 5, 0x1f4, 'pw_empirical_detect: status 5, a pc executed by two AIRs (pc 0x1f4)'),
    ("empirical.EmpiricalError", {}, 6, 0x0, 'pw_empirical_detect: status 6, fingerprint collisions under every seed'),
    ("empirical.EmpiricalError", {}, 7, 0x100000003, 'pw_empirical_detect: status 7, multiplicities on the bus that are no single receive with sends (air 1, row 3)'),
    ("execution_blocks.ExecutionBlocksError", {}, 2, 0x1000, 'pw_execution_blocks: status 2, the scratch bound is too small (4096 bytes needed)'),
    ("execution_blocks.ExecutionBlocksError", {}, 3, 0x11, 'pw_execution_blocks: status 3, not block-structured (position 17)'),
    ("execution_blocks.ExecutionBlocksError", {}, 4, 0x200000009, 'pw_execution_blocks: status 4, two rows with one time key (segment 2, timestamp 9)'),
    ("execution_blocks.ExecutionBlocksError", {}, 6, 0x0, 'pw_execution_blocks: status 6, fingerprint collisions under every seed'),
    ("execution_blocks.ExecutionBlocksError", {}, 7, 0x100000003, 'pw_execution_blocks: status 7, multiplicities on the bus that are no single receive with sends (air 1, row 3)'),
    ("execution_blocks.ExecutionBlocksError", {'from_traces': True}, 3, 0x200000009, 'pw_execution_blocks: status 3, not block-structured (segment 2, timestamp 9)'),
    ("execution_blocks.ExecutionBlocksError", {'from_traces': True}, 7, 0x100000003, 'pw_execution_blocks: status 7, multiplicities on the bus that are no single receive with sends (air 1, row 3)'),
    ("apc_calls.ApcCallsError", {}, 2, 0x1000, 'pw_apc_calls: status 2, the scratch bound is too small (4096 bytes needed)'),
    ("apc_calls.ApcCallsError", {}, 4, 0x200000009, 'pw_apc_calls: status 4, two rows with one time key (segment 2, timestamp 9)'),
    ("apc_calls.ApcCallsError", {}, 6, 0x0, 'pw_apc_calls: status 6, ?'),
    ("apc_calls.ApcCallsError", {}, 7, 0x100000003, 'pw_apc_calls: status 7, multiplicities on the bus that are no single receive with sends (air 1, row 3)'),
    ("apc_calls.ApcCallsError", {}, 8, 0xc00014000009, 'pw_apc_calls: status 8, a register tuple that is none (air 3, interaction 5, row 9)'),
    ("apc_calls.ApcCallsError", {}, 9, 0x7, 'pw_apc_calls: status 9, a requested register without a value (register 7)'),
    ("apc_calls.ApcCallsError", {}, 10, 0x7, 'pw_apc_calls: status 10, the initial registers contradicted by the first receive (register 7)'),
    ("apc_calls.ApcCallsError", {}, 11, 0x4, 'pw_apc_calls: status 11, ? (call 4)'),
    ("apc_calls.ApcCallsError", {}, 12, 0x6, 'pw_apc_calls: status 12, ? (position 6)'),
    ("execution_states.ExecutionStatesError", {}, 2, 0x1000, 'pw_execution_states: status 2, the scratch bound is too small (4096 bytes needed)'),
    ("execution_states.ExecutionStatesError", {}, 4, 0x200000009, 'pw_execution_states: status 4, two rows with one time key (segment 2, timestamp 9)'),
    ("execution_states.ExecutionStatesError", {}, 6, 0x0, 'pw_execution_states: status 6, ?'),
    ("execution_states.ExecutionStatesError", {}, 7, 0x100000003, 'pw_execution_states: status 7, multiplicities on the bus that are no single receive with sends (air 1, row 3)'),
    ("execution_states.ExecutionStatesError", {}, 8, 0xc00014000009, 'pw_execution_states: status 8, a register tuple that is none (air 3, interaction 5, row 9)'),
    ("execution_states.ExecutionStatesError", {}, 9, 0x7, 'pw_execution_states: status 9, a requested register without a value (register 7)'),
    ("execution_states.ExecutionStatesError", {}, 10, 0x7, 'pw_execution_states: status 10, the initial registers contradicted by the first receive (register 7)'),
    ("execution_states.ExecutionStatesError", {}, 11, 0x4, 'pw_execution_states: status 11, ? (call 4)'),
    ("execution_states.ExecutionStatesError", {}, 12, 0x6, 'pw_execution_states: status 12, ? (position 6)'),
    ("apc_sources.ApcSourcesError", {}, 2, 0x1000, 'pw_apc_sources: status 2, the scratch bound is too small (4096 bytes needed)'),
    ("apc_sources.ApcSourcesError", {}, 4, 0x200000009, 'pw_apc_sources: status 4, two rows with one time key (segment 2, timestamp 9)'),
    ("apc_sources.ApcSourcesError", {}, 6, 0x0, 'pw_apc_sources: status 6, ?'),
    ("apc_sources.ApcSourcesError", {}, 7, 0x100000003, 'pw_apc_sources: status 7, multiplicities on the bus that are no single receive with sends (air 1, row 3)'),
    ("apc_sources.ApcSourcesError", {}, 8, 0xc00014000009, 'pw_apc_sources: status 8, ? (air 3, interaction 5, row 9)'),
    ("apc_sources.ApcSourcesError", {}, 9, 0x7, 'pw_apc_sources: status 9, ? (register 7)'),
    ("apc_sources.ApcSourcesError", {}, 10, 0x7, 'pw_apc_sources: status 10, ? (register 7)'),
    ("apc_sources.ApcSourcesError", {}, 11, 0x4, 'pw_apc_sources: status 11, a call that ends after the execution (call 4)'),
    ("apc_sources.ApcSourcesError", {}, 12, 0x6, 'pw_apc_sources: status 12, two calls of one APC disagree on the AIR of an instruction (position 6)'),
    ("execution_segments.ExecutionSegmentsError", {}, 2, 0x1000, 'pw_execution_segments: status 2, the scratch bound is too small (4096 bytes needed)'),
    ("execution_segments.ExecutionSegmentsError", {}, 4, 0x200000009, 'pw_execution_segments: status 4, two rows with one time key (segment 2, timestamp 9)'),
    ("execution_segments.ExecutionSegmentsError", {}, 6, 0x0, 'pw_execution_segments: status 6, ?'),
    ("execution_segments.ExecutionSegmentsError", {}, 7, 0x100000003, 'pw_execution_segments: status 7, multiplicities on the bus that are no single receive with sends (air 1, row 3)'),
    ("execution_segments.ExecutionSegmentsError", {}, 8, 0xc00014000009, 'pw_execution_segments: status 8, ? (air 3, interaction 5, row 9)'),
    ("execution_segments.ExecutionSegmentsError", {}, 9, 0x7, 'pw_execution_segments: status 9, ? (register 7)'),
    ("execution_segments.ExecutionSegmentsError", {}, 10, 0x7, 'pw_execution_segments: status 10, ? (register 7)'),
    ("execution_segments.ExecutionSegmentsError", {}, 11, 0x4, 'pw_execution_segments: status 11, a call that ends after the execution (call 4)'),
    ("execution_segments.ExecutionSegmentsError", {}, 12, 0x6, 'pw_execution_segments: status 12, ? (position 6)'),
    ("execution_segments.ExecutionSegmentsError", {}, 13, 0x2, 'pw_execution_segments: status 13, nothing fits under max_cells (position 2)'),
    ("execution_segments.ExecutionSegmentsError", {}, 14, 0x2, 'pw_execution_segments: status 14, more than max_segments segments (position 2)'),
]


@pytest.mark.parametrize("name,kw,status,info,text", MESSAGES, ids=[f"{m[0].split('.')[1]}-{m[2]}{'-traces' if m[1] else ''}" for m in MESSAGES])
def test_messages_are_what_the_separate_classes_gave(name, kw, status, info, text):
    from powdr_amd import stage

    module, cls = name.split(".")
    e = getattr(importlib.import_module("powdr_amd." + module), cls)(status, info, **kw)
    assert str(e) == text
    assert (e.status, e.info) == (status, info) and isinstance(e, stage.StageError) and isinstance(e, ValueError)
    assert ("(" in text) == (status != 6)  # an undecoded status: no parentheses


def test_the_witness_codec():
    from powdr_amd import stage

    assert stage.pack_witness(3, 5, 9) == 0xC00014000009 and stage.unpack_witness(0xC00014000009) == (3, 5, 9)
    top = (2**18 - 1, 2**20 - 1, 2**26 - 1)
    assert stage.unpack_witness(stage.pack_witness(*top)) == top and stage.pack_witness(*top) == 2**64 - 1


class Destroy:
    def __init__(self):
        self.calls = []

    def __call__(self, handle):
        self.calls.append(handle)


def test_a_handle_is_destroyed_exactly_once():
    from powdr_amd import stage

    d = Destroy()
    h = stage.Handle(11, d)
    h.close()
    h.close()
    assert d.calls == [11] and h._h is None
    with stage.Handle(12, d) as h:
        assert h._h == 12 and d.calls == [11]
    h.close()
    assert d.calls == [11, 12]
    h = stage.Handle(13, d)
    h.close()
    del h
    gc.collect()
    assert d.calls == [11, 12, 13]
    h = stage.Handle(14, d)  # never closed: the collector's
    del h
    gc.collect()
    assert d.calls == [11, 12, 13, 14]


def test_the_result_classes_are_handles_and_refuse_use_after_close():
    from powdr_amd import apc_calls, apc_sources, execution_blocks, execution_segments, execution_states, stage

    for cls in (execution_blocks.ExecutionBlocks, execution_states.ExecutionStates, apc_calls.ApcCalls, apc_sources.ApcSources, execution_segments.ExecutionSegments):
        assert issubclass(cls, stage.Handle)
        assert not {"close", "__enter__", "__exit__", "__del__"} & set(vars(cls)), cls  # one copy, the base's
    d = Destroy()
    e = object.__new__(execution_blocks.ExecutionBlocks)  # (a real one needs a result of the library)
    stage.Handle.__init__(e, 15, d)
    e.close()
    with pytest.raises(ValueError, match="the execution blocks are closed"):
        e.count([0])
    assert d.calls == [15]


class StandIn:
    """what air_records reads of a Prover"""

    def __init__(self, handle):
        self._h = handle


def test_air_records_layout():
    from powdr_amd import prover, stage

    assert prover.PwSegmentAir is stage.PwSegmentAir and C.sizeof(stage.PwSegmentAir) == 24
    seg = [(StandIn(0x1000), 0x2000, 3), (StandIn(0x3000), 0x4000, 20), (StandIn(None), None, 0)]
    recs, numbers = stage.air_records(seg)
    assert numbers is None and len(recs) == 3
    assert [(r.prover, r.d_trace, r.log_height, r.flags) for r in recs] == [(0x1000, 0x2000, 3, 0), (0x3000, 0x4000, 20, 0), (None, None, 0, 0)]
    recs, numbers = stage.air_records(seg, segments=[7, 7, 2**32 - 1], flags=[1, 0, 1])
    assert [r.flags for r in recs] == [1, 0, 1] and list(numbers) == [7, 7, 2**32 - 1] and isinstance(numbers, C.Array) and numbers._type_ is C.c_uint32
    recs, numbers = stage.air_records([], segments=[])  # a pointer the C call may take: one zeroed record, one zero
    assert len(recs) == 1 and len(numbers) == 1 and (recs[0].prover, recs[0].d_trace, recs[0].log_height, recs[0].flags, numbers[0]) == (None, None, 0, 0, 0)
    for wrong in ([], [0], [0, 0, 0, 0]):
        with pytest.raises(AssertionError):
            stage.air_records(seg, segments=wrong)
    assert stage.is_air_list(seg) and stage.is_air_list(tuple(seg))
    assert not stage.is_air_list([]) and not stage.is_air_list([1, 2, 3]) and not stage.is_air_list([(1, 2, 3)]) and not stage.is_air_list(seg[0])


def test_minus_one_means_malformed_in_all_six_wrappers():
    from powdr_amd import abi, apc_calls, apc_sources, empirical, execution_blocks, execution_segments, execution_states, stage

    assert issubclass(stage.Malformed, abi.HipError) and issubclass(stage.Malformed, ValueError)
    assert str(stage.Malformed("pw_x")) == "pw_x: malformed arguments" and str(stage.Malformed("pw_x", " (why)")) == "pw_x: malformed arguments (why)"
    two = [(StandIn(None), None, 3), (StandIn(None), None, 3)]  # (the existing refusals' AIR list: NULL provers)
    wrappers = {
        "pw_empirical_detect": lambda: empirical.detect([], [(8, 2), (0, 2)]),  # an unsorted block table
        "pw_execution_blocks_from_pcs": lambda: execution_blocks.detect([], [(0, 2)], pc_step=0),  # a pc list with pc_step 0
        "pw_apc_calls_from_traces": lambda: apc_calls.select_calls(two, [apc_calls.Apc(0, 1, 1)], final_pc=0, segments=[0, 1]),  # two segment numbers
        "pw_execution_states_from_traces": lambda: execution_states.states_from_traces(two, [1], 0, segments=[0, 1]),
        "pw_apc_sources_from_traces": lambda: apc_sources.apply_calls([], [(0, 3, 6), (0, 0, 3)], [3]),  # a call list out of order
        "pw_execution_segments_from_traces": lambda: execution_segments.cut([], 32, 0),  # max_log_height of 32
    }
    for what, f in wrappers.items():
        with pytest.raises(stage.Malformed) as e:
            f()
        assert str(e.value) == f"{what}: malformed arguments"
    with pytest.raises(stage.Malformed, match="pw_trace_gather_rows: malformed arguments"):
        apc_sources.gather_rows([apc_sources.GatherJob(256, 8, 0, 512, 1024, 4)])
    with pytest.raises(abi.HipError, match="hipError 3"):
        stage.check(3, "pw_x")
    stage.check(0, "pw_x")


def u32(*v):
    return (C.c_uint32 * max(len(v), 1))(*v)


def u64(*v):
    return (C.c_uint64 * max(len(v), 1))(*v)


def entries():
    """the two entry points that take a call list, as f(cycles, n_apcs, ids, start, end, n_calls) -> (rc, status, handle) on no AIR"""
    from powdr_amd import apc_sources, execution_segments, stage

    limits = execution_segments.PwSegmentLimits(5, 0, 0, 0)
    return {
        "pw_apc_sources_from_traces": (lambda *calls: stage.raw(apc_sources.lib.pw_apc_sources_from_traces, None, None, 0, 0, *calls, 0, 1 << 30),
                                       apc_sources.lib.pw_apc_sources_destroy),
        "pw_execution_segments_from_traces": (lambda c, n_apcs, *calls: stage.raw(execution_segments.lib.pw_execution_segments_from_traces, None, None, 0, 0, 0, c, None, n_apcs,
                                                                                 *calls, C.byref(limits), 1 << 30), execution_segments.lib.pw_execution_segments_destroy),
    }


# cycle counts, n_apcs, apc ids, starts, ends, n_calls: the good list of test_every_refusal_that_needs_no_gpu is
# cycles (3, 2), ids (0, 1, 0), starts (0, 3, 5), ends (3, 5, 8)
BAD_CALL_LISTS = {
    "an id equal to n_apcs": (u32(3, 2), 2, u32(0, 2, 0), u64(0, 3, 5), u64(3, 5, 8), 3),
    "a call one longer than its cycle count": (u32(3, 2), 2, u32(0, 1, 0), u64(0, 3, 6), u64(3, 6, 9), 3),
    "a call one shorter than its cycle count": (u32(3, 2), 2, u32(0, 1, 0), u64(0, 3, 5), u64(3, 4, 8), 3),
    "a call that ends before it starts": (u32(3, 2), 2, u32(0, 1, 0), u64(0, 5, 5), u64(3, 3, 8), 3),
    "a call starting one before the previous call's end": (u32(3, 2), 2, u32(0, 1, 0), u64(0, 2, 5), u64(3, 4, 8), 3),
    "calls out of order": (u32(3, 2), 2, u32(0, 1, 0), u64(5, 3, 0), u64(8, 5, 3), 3),
    "a zero cycle count of an APC with calls": (u32(3, 0), 2, u32(0, 1, 0), u64(0, 3, 3), u64(3, 3, 6), 3),
    "a zero cycle count of an APC without calls": (u32(3, 0), 2, u32(0, 0, 0), u64(0, 3, 6), u64(3, 6, 9), 3),
    "no cycle counts": (None, 2, u32(0, 1, 0), u64(0, 3, 5), u64(3, 5, 8), 3),
    "no ids": (u32(3, 2), 2, None, u64(0, 3, 5), u64(3, 5, 8), 3),
    "no starts": (u32(3, 2), 2, u32(0, 1, 0), None, u64(3, 5, 8), 3),
    "no ends": (u32(3, 2), 2, u32(0, 1, 0), u64(0, 3, 5), None, 3),
    "2^31 APCs": (u32(3, 2), 1 << 31, u32(), u64(), u64(), 0),
    "2^31 calls": (u32(3, 2), 2, u32(0, 1, 0), u64(0, 3, 5), u64(3, 5, 8), 1 << 31),
}


@pytest.mark.parametrize("what", BAD_CALL_LISTS)
def test_a_bad_call_list_is_refused_by_both_entries(what):
    for name, (f, _) in entries().items():
        assert f(*BAD_CALL_LISTS[what]) == (-1, 0, 0, None), name


def test_an_empty_call_list_is_accepted_by_both_entries():
    for name, (f, destroy) in entries().items():
        for calls in ((u32(3, 2), 2, u32(), u64(), u64(), 0), (None, 0, None, None, None, 0)):
            rc, status, info, handle = f(*calls)
            assert (rc, status) == (0, 0) and handle, name
            destroy(handle)
