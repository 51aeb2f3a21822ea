// The bus half of the mock prover (include/powdr_prover.h pw_check_segment_buses): are the buses of a segment
// balanced tuple by tuple, and if not, which tuples are left over — on the raw traces, nothing committed.
//   pass A  bus_sum_kernel     per selected bus the LogUp sum over all AIRs, interactions and rows (the verdict), and n_active
//   pass B  bus_tally_kernel   one bus at a time: every active (air, interaction, row) adds its centred multiplicity to the slot of
//                              its tuple's fingerprint in an open-addressing table; bus_compact_kernel lists the slots whose sum is
//                              non-zero mod p; witness_args_kernel re-evaluates the tuple words at the slots' witness rows
// The table itself — the claim loop, the load rule, the sizing and the growth from a small first table — is bus_shared.hpp's; what is
// here is the table's payload (sum, witness, count).
// One lane per row, interactions evaluated by eval_span / DenominatorAcc exactly as logup_perm_kernel evaluates them.
#include "scratch.hpp"
#include "bus_witness_args.hpp"

namespace pw {

namespace {

using namespace bus;
using bb::Ext;
using pwj::DenominatorSeeds;
using pwj::denominator_seeds;

struct Unbalanced { u64 witness, count; uint32_t net, pad; };  // (the witness first: witness_args_kernel reads a list of these)

// al + bus + sum_j bl^(j+1) a_j + bl^(n+1) n: the denominator of the interaction's tuple on row r with its ARITY folded in, so that
// (a, b) and (a, b, 0) differ (the prover's own denominator, interaction_denominator of logup_kernels.hip, stops before the last term)
template <bool FAST>
__device__ __forceinline__ Ext tuple_denominator(const LogupInteraction& it, const LogupProgram& lp, const uint32_t* __restrict__ m, size_t stride,
                                                 size_t r, uint32_t* stk, const DenominatorSeeds& sd, const Ext* __restrict__ blpow) {
    pwj::DenominatorAcc acc(sd, it.bus_monty);
    for (uint32_t j = 0; j < it.n_args; ++j) acc.add(eval_span<FAST>(lp, it.first_span + 1 + j, m, stride, r, stk), blpow[j + 1]);
    acc.add(bb::to_monty(it.n_args), blpow[it.n_args + 1]);
    return acc.result();
}

// ---- pass A ---------------------------------------------------------------------------------------------------------------------
// acc[5 slot + k] += coordinate k of sum_{rows, interactions of the bus} m / d (k < 4; Montgomery words added as integers: a
// workgroup's share is below 2^40, the host reduces mod p), acc[5 slot + 4] += the number of non-zero multiplicities.
// A lane walks `rows_per_lane` rows (row = first + k * kBlock: coalesced) and keeps ONE running fraction per bus over all of them —
// (num, den) <- (num d + m den, den d), no degree limit since nothing is committed — so a bus costs one extension inversion per lane,
// not per row; an interaction whose multiplicity is zero on the row costs no argument evaluation. The per-lane values are added
// per wave (cross-lane shuffles), per workgroup (LDS) and then by five atomics per (workgroup, bus): never one atomic per row.
template <bool FAST>
__global__ __launch_bounds__(kBlock) void bus_sum_kernel(const uint32_t* __restrict__ m, size_t H, uint32_t rows_per_lane, LogupProgram lp,
                                                          const uint32_t* __restrict__ order, const BusSeg* __restrict__ segs, uint32_t n_segs,
                                                          Ext al, const Ext* __restrict__ blpow, u64* __restrict__ acc) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    __shared__ u64 red[kWaves][5];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kBlock * rows_per_lane + threadIdx.x;
    const DenominatorSeeds sd = denominator_seeds(al);
    for (uint32_t s = 0; s < n_segs; ++s) {
        const BusSeg sg = segs[s];
        Ext num = bb::ext_zero(), den = bb::ext_one();
        bool any = false;
        u64 active = 0;
        for (uint32_t k = 0; k < rows_per_lane; ++k) {
            const size_t r = first + (size_t)k * kBlock;
            if (r >= H) break;
            for (uint32_t i = sg.begin; i < sg.end; ++i) {
                const LogupInteraction it = lp.d_inter[order[i]];
                const uint32_t mu = eval_span<FAST>(lp, it.first_span, m, H, r, stk);
                if (mu == 0u) continue;
                ++active;
                const Ext d = tuple_denominator<FAST>(it, lp, m, H, r, stk, sd, blpow);
                if (any) {
                    num = bb::ext_add(bb::ext_mul(num, d), bb::ext_scale(den, mu));
                    den = bb::ext_mul(den, d);
                } else {
                    num = bb::ext_from_base(mu);
                    den = d;
                    any = true;
                }
            }
        }
        const Ext q = any ? bb::ext_mul(num, bb::ext_inv(den)) : bb::ext_zero();
        u64 v[5] = {q.c[0], q.c[1], q.c[2], q.c[3], active};
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) red[threadIdx.x >> 6][k] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < 5) {
            u64 t = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) t += red[w][threadIdx.x];
            if (t) atomicAdd(acc + 5 * (size_t)sg.slot + threadIdx.x, t);
        }
        __syncthreads();
    }
}

// ---- pass B ---------------------------------------------------------------------------------------------------------------------
struct Table { TableView v; u64 *wit, *sum, *cnt; };

// Every active (interaction, row) of ONE bus in one AIR: the slot of its tuple's fingerprint (the four words of the denominator: the
// two 64-bit key words of claim_slot, bus_shared.hpp) gets the centred multiplicity added, the packed witness min-ed in and its count
// bumped. Every lane stops early once *overflow is set: the host throws the table away.
template <bool FAST>
__global__ __launch_bounds__(kBlock) void bus_tally_kernel(const uint32_t* __restrict__ m, size_t H, LogupProgram lp, const uint32_t* __restrict__ order,
                                                            uint32_t begin, uint32_t end, uint32_t air, Ext al, const Ext* __restrict__ blpow, Table t,
                                                            uint32_t* __restrict__ overflow) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= H || __atomic_load_n(overflow, __ATOMIC_RELAXED)) return;
    const DenominatorSeeds sd = denominator_seeds(al);
    for (uint32_t i = begin; i < end; ++i) {
        const uint32_t idx = order[i];
        const LogupInteraction it = lp.d_inter[idx];
        const uint32_t mu = eval_span<FAST>(lp, it.first_span, m, H, r, stk);
        if (mu == 0u) continue;
        const Ext d = tuple_denominator<FAST>(it, lp, m, H, r, stk, sd, blpow);
        const u64 a = (u64)d.c[0] | ((u64)d.c[1] << 32), b = (u64)d.c[2] | ((u64)d.c[3] << 32);
        const u64 witness = pack_witness(air, idx, r);
        const long long cm = (long long)bb::centred(bb::from_monty(mu));
        const u64 s = claim_slot<2>(t.v, a, b, overflow);
        if (s == kEmpty) return;
        atomicAdd(t.sum + s, (u64)cm);
        atomicMin(t.wit + s, witness);
        atomicAdd(t.cnt + s, 1ull);
    }
}

// counts[0] = slots in use, counts[1] = slots whose sum is non-zero mod p; those are written to out[0 .. cap) in arrival order (the host
// sorts them by their tuples; cap = the count of a first, counting launch, so nothing is dropped)
__global__ __launch_bounds__(kBlock) void bus_compact_kernel(Table t, Unbalanced* __restrict__ out, u64 cap, u64* __restrict__ counts) {
    const u64 s = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (s > t.v.mask || t.v.k0[s] == kEmpty) return;
    const uint32_t net = sum_residue(t.sum[s]);
    if (!out) atomicAdd(counts, 1ull);
    if (net == 0) return;
    if (!out) { atomicAdd(counts + 1, 1ull); return; }
    const u64 at = atomicAdd(counts + 2, 1ull);
    if (at < cap) out[at] = Unbalanced{t.wit[s], t.cnt[s], net, 0u};
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct BusCtx : Scratch {
    Buf small{*this, kStays};  // accumulators | counters | class loads | challenge powers | bus runs | AIR table
    Buf table{*this}, list{*this}, args{*this};
    uint64_t stat_slots = 0, stat_occupied = 0, stat_inserted = 0, stat_tables = 0;
    void reset_stats() override { stat_slots = stat_occupied = stat_inserted = stat_tables = 0; }
};
thread_local BusCtx g_bus;

}  // namespace

}  // namespace pw

using namespace pw;

extern "C" size_t pw_bus_check_scratch_bytes(void) { return g_bus.held(); }
extern "C" size_t pw_bus_check_peak_bytes(void) { return g_bus.peak(); }
// for tools/bench_bus_check.py, deliberately not in the header: slots of the largest tally table kept, the most slots occupied in one
// table, the triples inserted over all tallied buses, the tables tallied into (attempts that overflowed included) — of the calling
// thread's last check (each NULL = skip)
extern "C" void pw_bus_check_last_stats(uint64_t* table_slots, uint64_t* occupied_slots, uint64_t* inserted, uint64_t* tables) {
    if (tables) *tables = g_bus.stat_tables;
    if (table_slots) *table_slots = g_bus.stat_slots;
    if (occupied_slots) *occupied_slots = g_bus.stat_occupied;
    if (inserted) *inserted = g_bus.stat_inserted;
}

extern "C" int pw_check_segment_buses(const PwSegmentAir* airs, size_t n_airs, const uint32_t* buses, size_t n_buses, uint64_t seed,
                                      size_t table_bytes, uint32_t flags, PwBusSummary* summaries, size_t summary_cap, size_t* n_summaries,
                                      PwBusTuple* tuples, size_t tuple_cap, size_t* n_tuples) {
    // ---- arguments: everything that can be refused is refused before the first GPU call
    if ((!airs && n_airs) || (!buses && n_buses) || (flags & ~PW_BUS_CHECK_TALLY_ALL)) return -1;
    if ((summaries != nullptr) != (summary_cap != 0) || (summaries && !n_summaries)) return -1;
    if ((!tuples && tuple_cap) || (tuples && !n_tuples)) return -1;
    if (!airs_well_formed(airs, n_airs)) return -1;
    std::vector<uint32_t> sel;
    if (n_buses) {
        for (size_t i = 0; i < n_buses; ++i) sel.push_back(buses[i] % bb::P);
    } else {
        for (size_t a = 0; a < n_airs; ++a)
            if (airs[a].prover->logup)
                for (const LogupInteraction& it : airs[a].prover->h_inter) sel.push_back(bb::from_monty(it.bus_monty));
    }
    std::sort(sel.begin(), sel.end());
    sel.erase(std::unique(sel.begin(), sel.end()), sel.end());
    const size_t n_sel = sel.size();
    if (summaries && n_sel > summary_cap) return -1;
    if (n_summaries) *n_summaries = n_sel;
    if (n_tuples) *n_tuples = 0;
    BusCtx& cx = g_bus;
    const ScratchCall call(cx);
    if (!n_sel) return 0;

    // ---- the AIRs that take part, their bus runs, the challenge powers
    struct BusPart { size_t air; std::vector<BusSeg> segs; size_t seg_off; const uint32_t* vals; };
    std::vector<BusPart> parts;
    std::vector<BusSeg> all_segs;
    uint32_t max_args = 0;
    for (size_t a = 0; a < n_airs; ++a) {
        PwProver* p = airs[a].prover;
        if (!p->logup || !p->n_inter) continue;
        PW_TRY(ensure_bus_order(p));
        BusPart part{a, {}, all_segs.size(), nullptr};
        for (size_t k = 0; k < p->h_bus_ids.size(); ++k) {
            const auto at = std::lower_bound(sel.begin(), sel.end(), p->h_bus_ids[k]);
            if (at == sel.end() || *at != p->h_bus_ids[k]) continue;
            part.segs.push_back(BusSeg{p->h_bus_starts[k], p->h_bus_starts[k + 1], (uint32_t)(at - sel.begin()), 0u});
        }
        if (part.segs.empty()) continue;
        max_args = std::max(max_args, p->max_args);
        all_segs.insert(all_segs.end(), part.segs.begin(), part.segs.end());
        parts.push_back(std::move(part));
    }
    uint64_t s = seed ^ 0x70775f6275736573ull;
    const Ext al = challenge(s), bl = challenge(s);
    std::vector<Ext> blpow(max_args + 2);
    blpow[0] = bb::ext_one();
    for (size_t j = 1; j < blpow.size(); ++j) blpow[j] = bb::ext_mul(blpow[j - 1], bl);

    // small: accumulators (5 u64 per bus) | the walker's head (counters: in use | unbalanced | written | unused) | powers | bus runs | AIR table
    const size_t off_head = n_sel * 5 * 8, off_pow = off_head + sizeof(WalkHead), off_seg = off_pow + blpow.size() * sizeof(Ext),
                 off_air = (off_seg + all_segs.size() * sizeof(BusSeg) + 15) & ~(size_t)15, small_bytes = off_air + n_airs * sizeof(AirDev);
    PW_TRY(cx.small.ensure(small_bytes));
    char* base = cx.small.as<char>();
    u64* d_acc = (u64*)base;
    WalkHead* d_head = (WalkHead*)(base + off_head);
    u64* d_counts = d_head->c.counts;
    const Ext* d_blpow = (const Ext*)(base + off_pow);
    const BusSeg* d_segs = (const BusSeg*)(base + off_seg);
    AirDev* d_airs = (AirDev*)(base + off_air);
    hipStream_t st = stream();
    PW_HIP_TRY(hipMemsetAsync(base, 0, off_pow, st));
    PW_HIP_TRY(hipMemcpyAsync(base + off_pow, blpow.data(), blpow.size() * sizeof(Ext), hipMemcpyHostToDevice, st));
    if (!all_segs.empty()) PW_HIP_TRY(hipMemcpyAsync(base + off_seg, all_segs.data(), all_segs.size() * sizeof(BusSeg), hipMemcpyHostToDevice, st));

    std::vector<AirDev> air_tab(n_airs, AirDev{nullptr, 0, LogupProgram{}});
    for (BusPart& part : parts) {
        const PwSegmentAir& A = airs[part.air];
        PW_TRY(stage_values(A, &part.vals));
        air_tab[part.air] = AirDev{part.vals, (u64)1 << A.log_height, program_of(A.prover)};
    }
    PW_HIP_TRY(hipMemcpyAsync(d_airs, air_tab.data(), n_airs * sizeof(AirDev), hipMemcpyHostToDevice, st));

    // ---- pass A
    {
        ScopedKernelTimer timer("bus_sum_kernel");
        for (const BusPart& part : parts) {
            const Walked w = walked(airs[part.air]);
            const uint32_t rows = airs[part.air].log_height >= 16 ? 4u : 1u;
            with_fast(w.lp, [&](auto fast) {
                hipLaunchKernelGGL(bus_sum_kernel<decltype(fast)::value>, dim3(div_up(w.H, (size_t)kBlock * rows)), dim3(kBlock), 0, st, part.vals, w.H, rows, w.lp,
                                   w.order, d_segs + part.seg_off, (uint32_t)part.segs.size(), al, d_blpow, d_acc);
            });
        }
    }
    PW_HIP_TRY(hipGetLastError());
    std::vector<u64> acc(n_sel * 5);
    PW_HIP_TRY(hipMemcpyAsync(acc.data(), d_acc, acc.size() * 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    std::vector<PwBusSummary> sums(n_sel);
    std::vector<bool> zero_sum(n_sel);
    for (size_t b = 0; b < n_sel; ++b) {
        bool z = true;
        for (int k = 0; k < 4; ++k) z = z && acc[5 * b + k] % bb::P == 0;
        zero_sum[b] = z;
        sums[b] = PwBusSummary{sel[b], z ? 0u : 2u, acc[5 * b + 4], 0};
    }

    // ---- pass B, one bus at a time
    size_t room = 0;
    bool room_known = false;
    size_t n_out = 0;
    for (size_t b = 0; b < n_sel; ++b) {
        if ((zero_sum[b] && !(flags & PW_BUS_CHECK_TALLY_ALL)) || !sums[b].n_active) continue;
        // the table's bound: the caller's, or by default half of the device's room (asked once per call)
        if (!table_bytes && !room_known) {
            room = call.bound(0);
            room_known = true;
        }
        uint32_t stride = 1;
        for (const BusPart& part : parts)
            for (const BusSeg& x : part.segs)
                if (x.slot == b)
                    for (uint32_t i = x.begin; i < x.end; ++i)
                        stride = std::max(stride, airs[part.air].prover->h_inter[airs[part.air].prover->h_bus_order[i]].n_args);
        // tally into tables that grow until one holds the bus (grow_table, bus_shared.hpp; that an overflowing tally is cheap has not been
        // measured: DESIGN.md §5i)
        Table T{};
        Grown g;
        PW_TRY(grow_table(
            cx.table, d_head, sums[b].n_active, kSlotBytes, table_bytes ? table_bytes : room, kStartSlots, "bus_table_clear",
            [&](u64* tb, const TableRule& rule) -> int {
                const u64 slots = rule.mask + 1;
                T = Table{TableView{rule, tb, tb + slots}, tb + 2 * slots, tb + 3 * slots, tb + 4 * slots};
                PW_HIP_TRY(hipMemsetAsync(tb, 0xFF, 3 * slots * 8, st));
                PW_HIP_TRY(hipMemsetAsync(tb + 3 * slots, 0, 2 * slots * 8, st));
                return 0;
            },
            [&] {
                ScopedKernelTimer timer("bus_tally_kernel");
                for (const BusPart& part : parts) {
                    const BusSeg* sg = nullptr;
                    for (const BusSeg& x : part.segs)
                        if (x.slot == b) sg = &x;
                    if (!sg) continue;
                    const Walked w = walked(airs[part.air]);
                    with_fast(w.lp, [&](auto fast) {
                        hipLaunchKernelGGL(bus_tally_kernel<decltype(fast)::value>, dim3(div_up(w.H, kBlock)), dim3(kBlock), 0, st, part.vals, w.H, w.lp, w.order,
                                           sg->begin, sg->end, (uint32_t)part.air, al, d_blpow, T, &d_head->c.overflow);
                    });
                }
            },
            [&] { hipLaunchKernelGGL(bus_compact_kernel, dim3(div_up(T.v.mask + 1, kBlock)), dim3(kBlock), 0, st, T, (Unbalanced*)nullptr, (u64)0, d_counts); }, &g));
        cx.stat_tables += g.tables;
        if (g.no_table) continue;  // (status 2 when the sum is not zero, balanced otherwise: as pass A left it)
        const u64 slots = g.slots;
        cx.stat_slots = std::max<uint64_t>(cx.stat_slots, slots);
        cx.stat_occupied = std::max<uint64_t>(cx.stat_occupied, g.c.counts[0]);
        if (g.overflowed()) continue;  // not localised
        cx.stat_inserted += sums[b].n_active;
        const u64 n_unb = g.c.counts[1];
        sums[b].status = n_unb ? 1u : 0u;
        sums[b].n_unbalanced = n_unb;
        if (!n_unb || !tuples || n_out >= tuple_cap) continue;
        // the unbalanced slots, their tuple words at the witness rows, sorted on the host
        PW_TRY(cx.list.ensure(n_unb * sizeof(Unbalanced)));
        PW_TRY(cx.args.ensure(n_unb * stride * 4));
        PW_HIP_TRY(hipMemsetAsync(cx.args.p, 0, n_unb * stride * 4, st));
        hipLaunchKernelGGL(bus_compact_kernel, dim3(div_up(slots, kBlock)), dim3(kBlock), 0, st, T, cx.list.as<Unbalanced>(), n_unb, d_counts);
        hipLaunchKernelGGL(witness_args_kernel, dim3(div_up(n_unb, kWaves)), dim3(kBlock), 0, st, (const u64*)cx.list.p, (uint32_t)(sizeof(Unbalanced) / 8), n_unb,
                           (const AirDev*)d_airs, stride, cx.args.as<uint32_t>(), (uint32_t*)nullptr);
        PW_HIP_TRY(hipGetLastError());
        std::vector<Unbalanced> list(n_unb);
        std::vector<uint32_t> args(n_unb * stride);
        PW_HIP_TRY(hipMemcpyAsync(list.data(), cx.list.p, n_unb * sizeof(Unbalanced), hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(args.data(), cx.args.p, args.size() * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        auto n_args_of = [&](const Unbalanced& u) {
            const Witness w = unpack_witness(u.witness);
            return airs[w.air].prover->h_inter[w.inter].n_args;
        };
        std::vector<size_t> idx(n_unb);
        for (size_t i = 0; i < n_unb; ++i) idx[i] = i;
        // (only the first tuple_cap - n_out in order are reported: a bus without receivers has millions of leftover tuples)
        const size_t keep = std::min<size_t>(n_unb, tuple_cap - n_out);
        std::partial_sort(idx.begin(), idx.begin() + keep, idx.end(), [&](size_t x, size_t y) {
            const uint32_t nx = n_args_of(list[x]), ny = n_args_of(list[y]);
            if (nx != ny) return nx < ny;
            const uint32_t *ax = &args[x * stride], *ay = &args[y * stride];
            if (!std::equal(ax, ax + nx, ay)) return std::lexicographical_compare(ax, ax + nx, ay, ay + nx);
            return list[x].witness < list[y].witness;  // (equal tuples in two slots: only after a fingerprint collision)
        });
        for (size_t k = 0; k < keep; ++k, ++n_out) {
            const Unbalanced& u = list[idx[k]];
            PwBusTuple& t = tuples[n_out];
            memset(&t, 0, sizeof t);
            t.bus = sel[b];
            t.n_args = n_args_of(u);
            for (uint32_t j = 0; j < t.n_args && j < PW_BUS_MAX_ARGS; ++j) t.args[j] = args[idx[k] * stride + j];
            t.net_multiplicity = u.net;
            const Witness w = unpack_witness(u.witness);
            t.air = w.air;
            t.interaction = w.inter;
            t.row = w.row;
            t.n_contributions = u.count;
        }
    }
    if (summaries) memcpy(summaries, sums.data(), n_sel * sizeof(PwBusSummary));
    if (n_tuples) *n_tuples = n_out;
    return (int)hipGetLastError();
}
