// The bus half of the mock prover (include/powdr_prover.h pw_check_segment_buses): are the buses of a segment
// balanced tuple by tuple, and if not, which tuples are left over — on the raw traces, nothing committed.
//   pass A  bus_sum_kernel     per selected bus the LogUp sum over all AIRs, interactions and rows (the verdict), and n_active
//   pass B  bus_tally_kernel   one bus at a time: every active (air, interaction, row) adds its centred multiplicity to the slot of
//                              its tuple's fingerprint in an open-addressing table; bus_compact_kernel lists the slots whose sum is
//                              non-zero mod p; bus_args_kernel re-evaluates the tuple words at the slots' witness rows. The table
//                              starts small and is quadrupled (and the bus tallied again) until it holds the bus or reaches its bound
// One lane per row, interactions evaluated by eval_span / DenominatorAcc exactly as logup_perm_kernel evaluates them.
#include "bus_shared.hpp"

namespace pw {

namespace {

using namespace bus;
using bb::Ext;
using pwj::DenominatorSeeds;
using pwj::denominator_seeds;

struct Unbalanced { u64 witness, count; uint32_t net, pad; };

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
struct Table { u64 *k0, *k1, *wit, *sum, *cnt; u64 mask; u64* load; u64 class_mask, class_cap; };

// Every active (interaction, row) of ONE bus in one AIR: the slot of its tuple's fingerprint (the four words of the denominator: two
// 64-bit key halves, each claimed by a compare-and-swap; a slot whose first half matches and whose second does not belongs to another
// tuple: keep probing) gets the centred multiplicity added, the packed witness min-ed in and its count bumped. Keys never change once
// set, so every contribution of a tuple ends in the same slot whatever the order of arrival. The lane that claims a fresh slot counts
// it in the slot's class; a class past its cap sets *overflow (and so does a lane that has seen every slot taken by other tuples: only
// tables of fewer than 8 slots get that far). With linear probing the SET of taken slots does not depend on the order of arrival and
// only grows with the tuples inserted, so whether a class passes its cap — *overflow — is a function of the traces and the table size
// alone. Every lane stops early once it is set: the host throws the table away.
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
        const u64 h = slot_hash(a, b);
        bool done = false;
        for (u64 n = 0; n <= t.mask; ++n) {
            const u64 s = (h + n) & t.mask;
            u64 ka = __atomic_load_n(t.k0 + s, __ATOMIC_RELAXED);
            if (ka == kEmpty) {
                ka = atomicCAS(t.k0 + s, kEmpty, a);
                if (ka == kEmpty) {
                    ka = a;
                    if (atomicAdd(t.load + (s & t.class_mask) * kLoadStride, 1ull) >= t.class_cap) atomicOr(overflow, 1u);
                }
            }
            if (ka == a) {
                u64 kb = __atomic_load_n(t.k1 + s, __ATOMIC_RELAXED);
                if (kb == kEmpty) {
                    kb = atomicCAS(t.k1 + s, kEmpty, b);
                    if (kb == kEmpty) kb = b;
                }
                if (kb == b) {
                    atomicAdd(t.sum + s, (u64)cm);
                    atomicMin(t.wit + s, witness);
                    atomicAdd(t.cnt + s, 1ull);
                    done = true;
                    break;
                }
            }
            if ((n & 63) == 63 && __atomic_load_n(overflow, __ATOMIC_RELAXED)) break;
        }
        if (!done) {
            atomicOr(overflow, 1u);
            return;
        }
    }
}

// counts[0] = slots in use, counts[1] = slots whose sum is non-zero mod p; those are written to out[0 .. cap) in arrival order (the host
// sorts them by their tuples; cap = the count of a first, counting launch, so nothing is dropped)
__global__ __launch_bounds__(kBlock) void bus_compact_kernel(Table t, Unbalanced* __restrict__ out, u64 cap, u64* __restrict__ counts) {
    const u64 s = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (s > t.mask || t.k0[s] == kEmpty) return;
    const long long sum = (long long)t.sum[s];
    long long net = sum % (long long)bb::P;
    if (net < 0) net += (long long)bb::P;
    if (!out) atomicAdd(counts, 1ull);
    if (net == 0) return;
    if (!out) { atomicAdd(counts + 1, 1ull); return; }
    const u64 at = atomicAdd(counts + 2, 1ull);
    if (at < cap) out[at] = Unbalanced{t.wit[s], t.cnt[s], (uint32_t)net, 0u};
}

// args[e * stride + j] = argument j (canonical) of the interaction and row entry e's witness names; one wave per entry, every lane
// of it evaluating the same program on the same row (the interpreter wants wave-uniform code; the lists are short)
__global__ __launch_bounds__(kBlock) void bus_args_kernel(const Unbalanced* __restrict__ list, u64 n, const AirDev* __restrict__ airs, uint32_t stride,
                                                           uint32_t* __restrict__ args) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const u64 e = (u64)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (e >= n) return;
    const u64 w = list[e].witness;
    const AirDev a = airs[w >> (kRowBits + kInterBits)];
    const uint32_t idx = (uint32_t)(w >> kRowBits) & ((1u << kInterBits) - 1u);
    const size_t r = (size_t)(w & ((1ull << kRowBits) - 1ull));
    const LogupInteraction it = a.lp.d_inter[idx];
    for (uint32_t j = 0; j < it.n_args && j < stride; ++j) {
        const uint32_t v = a.lp.d_forms ? eval_span<true>(a.lp, it.first_span + 1 + j, a.m, (size_t)a.H, r, stk)
                                        : eval_span<false>(a.lp, it.first_span + 1 + j, a.m, (size_t)a.H, r, stk);
        if ((threadIdx.x & 63) == 0) args[e * stride + j] = bb::from_monty(v);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct BusCtx {
    DeviceBuf small;               // accumulators | counters | class loads | challenge powers | bus runs | AIR table: stays
    DeviceBuf table, list, args;   // released before the call returns, on every path (Released below)
    size_t peak = 0;
    uint64_t stat_slots = 0, stat_occupied = 0, stat_inserted = 0, stat_tables = 0;
    size_t held() const { return small.bytes + table.bytes + list.bytes + args.bytes; }
    void note() { peak = std::max(peak, held()); }
};
thread_local BusCtx g_bus;
struct Released {
    BusCtx& cx;
    ~Released() { cx.table.release(); cx.list.release(); cx.args.release(); }
};

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
Ext challenge(uint64_t& s) {
    Ext e;
    for (int k = 0; k < 4; ++k) e.c[k] = bb::to_monty((uint32_t)(splitmix(s) % bb::P));
    return e;
}

}  // namespace

}  // namespace pw

using namespace pw;

extern "C" size_t pw_bus_check_scratch_bytes(void) { return g_bus.held(); }
extern "C" size_t pw_bus_check_peak_bytes(void) { return g_bus.peak; }
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
    cx.peak = 0;
    cx.stat_slots = cx.stat_occupied = cx.stat_inserted = cx.stat_tables = 0;
    if (!n_sel) return 0;

    (void)hipGetLastError();
    // ---- the AIRs that take part, their bus runs, the challenge powers
    struct Part { size_t air; std::vector<BusSeg> segs; size_t seg_off; const uint32_t* vals; };
    std::vector<Part> parts;
    std::vector<BusSeg> all_segs;
    uint32_t max_args = 0;
    for (size_t a = 0; a < n_airs; ++a) {
        PwProver* p = airs[a].prover;
        if (!p->logup || !p->n_inter) continue;
        PW_TRY(ensure_bus_order(p));
        Part part{a, {}, all_segs.size(), nullptr};
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

    // small: accumulators (5 u64 per bus) | counters (4 u64) | overflow (+ padding, 16 bytes) | class loads | powers | bus runs | AIR table
    const size_t load_bytes = kMaxClasses * kLoadStride * 8;
    const size_t off_cnt = n_sel * 5 * 8, off_ovf = off_cnt + 32, off_load = off_ovf + 16, off_pow = off_load + load_bytes, off_seg = off_pow + blpow.size() * sizeof(Ext),
                 off_air = (off_seg + all_segs.size() * sizeof(BusSeg) + 15) & ~(size_t)15, small_bytes = off_air + n_airs * sizeof(AirDev);
    const Released released{cx};
    PW_TRY(cx.small.ensure(small_bytes));
    cx.note();
    char* base = cx.small.as<char>();
    u64* d_acc = (u64*)base;
    u64* d_counts = (u64*)(base + off_cnt);
    uint32_t* d_ovf = (uint32_t*)(base + off_ovf);
    u64* d_load = (u64*)(base + off_load);
    const Ext* d_blpow = (const Ext*)(base + off_pow);
    const BusSeg* d_segs = (const BusSeg*)(base + off_seg);
    AirDev* d_airs = (AirDev*)(base + off_air);
    hipStream_t st = stream();
    PW_HIP_TRY(hipMemsetAsync(base, 0, off_pow, st));
    PW_HIP_TRY(hipMemcpyAsync(base + off_pow, blpow.data(), blpow.size() * sizeof(Ext), hipMemcpyHostToDevice, st));
    if (!all_segs.empty()) PW_HIP_TRY(hipMemcpyAsync(base + off_seg, all_segs.data(), all_segs.size() * sizeof(BusSeg), hipMemcpyHostToDevice, st));

    std::vector<AirDev> air_tab(n_airs, AirDev{nullptr, 0, LogupProgram{}});
    for (Part& part : parts) {
        const PwSegmentAir& A = airs[part.air];
        PW_TRY(stage_values(A, &part.vals));
        air_tab[part.air] = AirDev{part.vals, (u64)1 << A.log_height, program_of(A.prover)};
    }
    PW_HIP_TRY(hipMemcpyAsync(d_airs, air_tab.data(), n_airs * sizeof(AirDev), hipMemcpyHostToDevice, st));

    // ---- pass A
    {
        ScopedKernelTimer timer("bus_sum_kernel");
        for (const Part& part : parts) {
            const PwSegmentAir& A = airs[part.air];
            const PwProver* p = A.prover;
            const size_t H = (size_t)1 << A.log_height;
            const uint32_t* vals = part.vals;
            const uint32_t rows = A.log_height >= 16 ? 4u : 1u;
            const LogupProgram lp = program_of(p);
            const dim3 grid(div_up(H, (size_t)kBlock * rows));
            if (lp.d_forms)
                hipLaunchKernelGGL(bus_sum_kernel<true>, grid, dim3(kBlock), 0, st, vals, H, rows, lp, (const uint32_t*)p->bus_order.p, d_segs + part.seg_off,
                                   (uint32_t)part.segs.size(), al, d_blpow, d_acc);
            else
                hipLaunchKernelGGL(bus_sum_kernel<false>, grid, dim3(kBlock), 0, st, vals, H, rows, lp, (const uint32_t*)p->bus_order.p, d_segs + part.seg_off,
                                   (uint32_t)part.segs.size(), al, d_blpow, d_acc);
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
        // the largest table this bus may get: a power of two of slots, at most twice the active triples (no bus needs more), within the
        // caller's bound, or by default half of the device's room
        u64 max_slots = 1024;
        while (max_slots < 2 * sums[b].n_active) max_slots <<= 1;
        size_t bound = table_bytes;
        if (!bound) {
            if (!room_known) {
                size_t avail = 0;
                room = device_room(cx.held(), &avail) ? avail / 2 : (size_t)1 << 30;
                room_known = true;
            }
            bound = room;
        }
        while (max_slots && max_slots * kSlotBytes > bound) max_slots >>= 1;
        if (!max_slots) continue;  // (status 2 when the sum is not zero, balanced otherwise: as pass A left it)
        uint32_t stride = 1;
        for (const Part& part : parts)
            for (const BusSeg& x : part.segs)
                if (x.slot == b)
                    for (uint32_t i = x.begin; i < x.end; ++i)
                        stride = std::max(stride, airs[part.air].prover->h_inter[airs[part.air].prover->h_bus_order[i]].n_args);
        // tally into a small table first and into one four times as large while the bus overflows it: lookup buses repeat a few hundred
        // thousand tuples thousands of times, so the active count says little about the table a bus needs. What is reported depends on
        // the LAST table alone. An overflowing tally stops early (every lane leaves once the overflow word is set), which should keep the
        // attempts before the last one cheap; that has not been measured.
        u64 slots = std::min(max_slots, kStartSlots);
        u64 counts[6] = {0, 0, 0, 0, 1, 0};  // in use | unbalanced | written | (unused) | overflow word
        Table T{};
        for (;;) {
            // a table the device cannot give is a table too small: try half, never an error
            int erc;
            while ((erc = cx.table.ensure(slots * kSlotBytes)) != 0) {
                (void)hipGetLastError();
                if (erc != (int)hipErrorOutOfMemory) return erc;
                if (slots <= 1) break;
                max_slots = slots >>= 1;
            }
            if (!cx.table.p) break;
            cx.note();
            u64* tb = cx.table.as<u64>();
            const u64 classes = std::min<u64>(kMaxClasses, std::max<u64>(1, slots / kMinClassSlots)), per_class = slots / classes;
            T = Table{tb, tb + slots, tb + 2 * slots, tb + 3 * slots, tb + 4 * slots, slots - 1, d_load, classes - 1, per_class - per_class / 8};
            {
                ScopedKernelTimer timer("bus_table_clear");
                PW_HIP_TRY(hipMemsetAsync(tb, 0xFF, 3 * slots * 8, st));
                PW_HIP_TRY(hipMemsetAsync(tb + 3 * slots, 0, 2 * slots * 8, st));
                PW_HIP_TRY(hipMemsetAsync(d_counts, 0, 48 + load_bytes, st));  // counters, the overflow word, the class loads
            }
            {
                ScopedKernelTimer timer("bus_tally_kernel");
                for (const Part& part : parts) {
                    const BusSeg* sg = nullptr;
                    for (const BusSeg& x : part.segs)
                        if (x.slot == b) sg = &x;
                    if (!sg) continue;
                    const PwSegmentAir& A = airs[part.air];
                    const PwProver* p = A.prover;
                    const size_t H = (size_t)1 << A.log_height;
                    const LogupProgram lp = program_of(p);
                    const dim3 grid(div_up(H, kBlock));
                    if (lp.d_forms)
                        hipLaunchKernelGGL(bus_tally_kernel<true>, grid, dim3(kBlock), 0, st, part.vals, H, lp, (const uint32_t*)p->bus_order.p, sg->begin,
                                           sg->end, (uint32_t)part.air, al, d_blpow, T, d_ovf);
                    else
                        hipLaunchKernelGGL(bus_tally_kernel<false>, grid, dim3(kBlock), 0, st, part.vals, H, lp, (const uint32_t*)p->bus_order.p, sg->begin,
                                           sg->end, (uint32_t)part.air, al, d_blpow, T, d_ovf);
                }
            }
            hipLaunchKernelGGL(bus_compact_kernel, dim3(div_up(slots, kBlock)), dim3(kBlock), 0, st, T, (Unbalanced*)nullptr, (u64)0, d_counts);
            PW_HIP_TRY(hipGetLastError());
            PW_HIP_TRY(hipMemcpyAsync(counts, d_counts, 48, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            ++cx.stat_tables;
            if (!(uint32_t)counts[4] || slots >= max_slots) break;
            slots = std::min(max_slots, slots * 4);
        }
        if (!cx.table.p) continue;  // no table at all: as pass A left it
        cx.stat_slots = std::max<uint64_t>(cx.stat_slots, slots);
        cx.stat_occupied = std::max<uint64_t>(cx.stat_occupied, counts[0]);
        if ((uint32_t)counts[4]) continue;  // overflow: not localised
        cx.stat_inserted += sums[b].n_active;
        const u64 n_unb = counts[1];
        sums[b].status = n_unb ? 1u : 0u;
        sums[b].n_unbalanced = n_unb;
        if (!n_unb || !tuples || n_out >= tuple_cap) continue;
        // the unbalanced slots, their tuple words at the witness rows, sorted on the host
        PW_TRY(cx.list.ensure(n_unb * sizeof(Unbalanced)));
        PW_TRY(cx.args.ensure(n_unb * stride * 4));
        cx.note();
        PW_HIP_TRY(hipMemsetAsync(cx.args.p, 0, n_unb * stride * 4, st));
        hipLaunchKernelGGL(bus_compact_kernel, dim3(div_up(slots, kBlock)), dim3(kBlock), 0, st, T, cx.list.as<Unbalanced>(), n_unb, d_counts);
        hipLaunchKernelGGL(bus_args_kernel, dim3(div_up(n_unb, kWaves)), dim3(kBlock), 0, st, cx.list.as<Unbalanced>(), n_unb, d_airs, stride,
                           cx.args.as<uint32_t>());
        PW_HIP_TRY(hipGetLastError());
        std::vector<Unbalanced> list(n_unb);
        std::vector<uint32_t> args(n_unb * stride);
        PW_HIP_TRY(hipMemcpyAsync(list.data(), cx.list.p, n_unb * sizeof(Unbalanced), hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(args.data(), cx.args.p, args.size() * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        auto n_args_of = [&](const Unbalanced& u) {
            const PwProver* p = airs[u.witness >> (kRowBits + kInterBits)].prover;
            return p->h_inter[(u.witness >> kRowBits) & ((1u << kInterBits) - 1u)].n_args;
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
            t.air = (uint32_t)(u.witness >> (kRowBits + kInterBits));
            t.interaction = (uint32_t)(u.witness >> kRowBits) & ((1u << kInterBits) - 1u);
            t.row = u.witness & ((1ull << kRowBits) - 1ull);
            t.n_contributions = u.count;
        }
    }
    if (summaries) memcpy(summaries, sums.data(), n_sel * sizeof(PwBusSummary));
    if (n_tuples) *n_tuples = n_out;
    return (int)hipGetLastError();
}
