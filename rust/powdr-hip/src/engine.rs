//! The third engine beside `BabyBearPoseidon2CpuEngine` / `BabyBearPoseidon2GpuEngine` (openvm/src/lib.rs:69-95) and its
//! builder / prover-extension wiring (lib.rs:133-166 `SpecializedConfigGpuBuilder`, :217-269 `PowdrGpuProverExt`).
//!
//! The `StarkEngine` / `ProverBackend` / `ProverDevice` traits are defined in the EXTERNAL `openvm-stark-backend`; what
//! is evidenced in the powdr checkout is: `StarkEngine<SC = .., PB = .., PD = ..>` (lib.rs:175,286), `ProverBackend{Matrix}`
//! (cuda/mod.rs:404), `engine.prove(pk, ProvingContext{per_trace: [(air_id, AirProvingContext)]})`
//! (trace_generation.rs:97-139, empirical_constraints.rs:131). The impl below follows that surface; method names beyond
//! it are marked `// (EXTERNAL trait)`.
use crate::chip::{PowdrChipHip, PowdrPeripheryInstancesHip};
use crate::device::{DeviceBuffer, DeviceMatrix, HipError, MemCopyH2D};
use crate::ffi;
use std::marker::PhantomData;

use openvm_circuit::arch::{
    AirInventory, ChipInventory, ChipInventoryError, DenseRecordArena, VmBuilder, VmChipComplex, VmProverExtension,
};
use openvm_stark_backend::prover::{AirProvingContext, ProverBackend, ProvingContext};
use openvm_stark_backend::{keygen::types::MultiStarkProvingKey, StarkEngine};
use openvm_stark_backend::p3_field::PrimeField32; // (as_canonical_u32 of the public values)
use openvm_stark_sdk::p3_baby_bear::BabyBear;
use crate::isa_hip::OpenVmIsaHip;
use powdr_openvm::isa::OpenVmISA;
use powdr_openvm::powdr_extension::{chip::PowdrAir, PowdrExtension};
use powdr_openvm::{BabyBearSC, PeripheryBusIds, SpecializedConfig};

/// `ProverBackend` with column-major device matrices in HBM (the CUDA engine's `GpuBackend`, lib.rs:79)
pub struct HipBackend;
impl ProverBackend for HipBackend {
    type Matrix = DeviceMatrix<BabyBear>;
    // (EXTERNAL trait) the remaining associated types (Val, Challenge, Commitment, ...) are BabyBearSC's
}

/// One prover object per AIR of the proving key, created at key generation from the AIR's constraint programs and
/// bus interactions (what `PowdrAir::eval` pushes through the symbolic builder, chip.rs:94-130).
pub struct HipAirProver {
    pub handle: *mut ffi::PwProver,
    pub width: u32,
}
impl Drop for HipAirProver {
    fn drop(&mut self) {
        unsafe { ffi::pw_prover_destroy(self.handle) }
    }
}

pub struct HipEngine {
    pub config: ffi::PwStarkConfig,
    /// indexed by air_id of the `MultiStarkProvingKey`
    pub provers: Vec<HipAirProver>,
}

/// The proof of one segment: ONE pw-stark v1 proof (magic PWS3) over all AIRs (include/powdr_prover.h).
pub struct HipSegmentProof {
    pub air_ids: Vec<usize>,
    pub log_heights: Vec<u32>,
    pub words: Vec<u32>,
}

impl HipEngine {
    /// keygen-side construction: `programs[air_id]` = (width, post-fix constraint bytecode, spans, interaction tables)
    /// — for APC AIRs `powdr_apc_compile_constraints` / `powdr_apc_compile_bus(apc, 1)` produce exactly these from the APC.
    pub fn new(config: ffi::PwStarkConfig, programs: &[AirProgram]) -> Self {
        let provers = programs
            .iter()
            .map(|p| {
                // an AIR whose constraints read the next row or a row selector (`main.row_slice(1)`, `when_first_row()`,
                // `when_transition()`) takes the row layout; the others keep the plain entry and its words
                let rows = p.reads_rows();
                let handle = unsafe {
                    if p.n_public > 0 {
                        // public values (`builder.public_values()`): operands behind the row layout, set per segment
                        ffi::pw_prover_create_public(
                            &config, p.width, 0, 0, core::ptr::null(), p.n_public, p.cons_bytecode.as_ptr(), p.cons_bytecode.len(),
                            p.cons_spans.as_ptr(), p.cons_spans.len() / 2, p.interactions.as_ptr(), p.interactions.len() / 3,
                            p.inter_spans.as_ptr(), p.inter_spans.len() / 2, p.inter_bytecode.as_ptr(), p.inter_bytecode.len(),
                        )
                    } else if rows {
                        ffi::pw_prover_create_transition(
                            &config, p.width, 0, 0, core::ptr::null(), p.cons_bytecode.as_ptr(), p.cons_bytecode.len(),
                            p.cons_spans.as_ptr(), p.cons_spans.len() / 2, p.interactions.as_ptr(), p.interactions.len() / 3,
                            p.inter_spans.as_ptr(), p.inter_spans.len() / 2, p.inter_bytecode.as_ptr(), p.inter_bytecode.len(),
                        )
                    } else {
                        ffi::pw_prover_create_logup(
                            &config, p.width, p.cons_bytecode.as_ptr(), p.cons_bytecode.len(), p.cons_spans.as_ptr(),
                            p.cons_spans.len() / 2, p.interactions.as_ptr(), p.interactions.len() / 3, p.inter_spans.as_ptr(),
                            p.inter_spans.len() / 2, p.inter_bytecode.as_ptr(), p.inter_bytecode.len(),
                        )
                    }
                };
                // (the row-layout entry also refuses a constraint above degree 3 by Plonky3's rule: next-row columns and the
                // first / last row selectors count 1, is_transition 0)
                assert!(!handle.is_null(), "pw_prover_create_logup / _transition failed");
                // the reference's degree bound 2 * DEFAULT_APP_LOG_BLOWUP + 1 = 3 (lib.rs:97-101), by that rule
                assert!(unsafe { ffi::pw_prover_max_constraint_degree(handle) } <= 3, "constraint degree above the blow-up-2 bound");
                HipAirProver { handle, width: p.width }
            })
            .collect();
        Self { config, provers }
    }

    /// `engine.prove(pk, ctx)` (trace_generation.rs:136-139): ONE call per segment with the traces of all chips, one proof.
    pub fn prove_segment(&self, ctx: &ProvingContext<HipBackend>) -> Result<HipSegmentProof, HipError> {
        self.prove_segment_impl(ctx, false)
    }

    /// The reference's `engine.prove` takes the context BY VALUE: every chip moved its `common_main` into it
    /// (cuda/mod.rs:415-419). Owning the matrices lets an AIR that has to be streamed keep its coefficient arrays in the trace's
    /// own buffer (`pw_prove_segment_consuming`); the matrices are dropped with `ctx` when this returns.
    pub fn prove_segment_owned(&self, ctx: ProvingContext<HipBackend>) -> Result<HipSegmentProof, HipError> {
        self.prove_segment_impl(&ctx, true)
    }

    fn prove_segment_impl(&self, ctx: &ProvingContext<HipBackend>, hand_over: bool) -> Result<HipSegmentProof, HipError> {
        let mut airs = vec![];
        let mut air_ids = vec![];
        let mut log_heights = vec![];
        for (air_id, air_ctx) in &ctx.per_trace {
            let m: &DeviceMatrix<BabyBear> = &air_ctx.common_main;
            if m.height() == 0 {
                continue; // an APC that was not called in this segment
            }
            assert!(m.height().is_power_of_two() && m.width() as u32 == self.provers[*air_id].width);
            let log_h = m.height().trailing_zeros();
            // `AirProvingContext.public_values` (canonical words): the prover keeps a copy and the proof snapshots it when it begins
            if unsafe { ffi::pw_prover_n_public(self.provers[*air_id].handle) } > 0 {
                let pv: Vec<u32> = air_ctx.public_values.iter().map(|x| x.as_canonical_u32()).collect();
                let rc = unsafe { ffi::pw_prover_set_public_values(self.provers[*air_id].handle, pv.as_ptr(), pv.len()) };
                assert!(rc == 0, "AIR {air_id}: {} public values do not match the AIR's count", pv.len());
            }
            airs.push(ffi::PwSegmentAir {
                prover: self.provers[*air_id].handle,
                d_trace: m.buffer().as_ptr() as *const u32,
                log_height: log_h,
                flags: if hand_over { ffi::PW_AIR_HAND_OVER } else { 0 },
            });
            air_ids.push(*air_id);
            log_heights.push(log_h);
        }
        let mut words: *const u32 = core::ptr::null();
        let mut n_words = 0usize;
        // logup = 1: the bus interactions of every AIR are inside the proof; the cumulative sums must cancel
        HipError::from_result(unsafe {
            if hand_over {
                ffi::pw_prove_segment_consuming(airs.as_ptr(), airs.len(), 1, &mut words, &mut n_words)
            } else {
                ffi::pw_prove_segment(airs.as_ptr(), airs.len(), 1, &mut words, &mut n_words)
            }
        })?;
        let words = unsafe { std::slice::from_raw_parts(words, n_words) }.to_vec();
        Ok(HipSegmentProof { air_ids, log_heights, words })
    }

    /// The `PwSegmentAir` list of a context: its AIRs with a non-empty trace, in order, nothing handed over.
    fn segment_airs(&self, ctx: &ProvingContext<HipBackend>) -> Vec<ffi::PwSegmentAir> {
        ctx.per_trace.iter().filter(|(_, c)| c.common_main.height() != 0).map(|(air_id, c)| {
            let m: &DeviceMatrix<BabyBear> = &c.common_main;
            ffi::PwSegmentAir {
                prover: self.provers[*air_id].handle,
                d_trace: m.buffer().as_ptr() as *const u32,
                log_height: m.height().trailing_zeros(),
                flags: 0,
            }
        }).collect()
    }

    /// The bus half of `debug_proving_ctx` (`prove_mock`, openvm-riscv/src/lib.rs:288-294) on the device: every bus of the segment
    /// balanced tuple by tuple, or the tuples that are not, each with the (air, interaction, row) of one contribution. Nothing is
    /// committed; `bus_ids` empty = every bus the AIRs mention. `air` of a tuple indexes the AIRs of `ctx` with a non-empty trace.
    pub fn debug_segment_buses(&self, ctx: &ProvingContext<HipBackend>, bus_ids: &[u32], tuple_cap: usize)
                               -> Result<(Vec<ffi::PwBusSummary>, Vec<ffi::PwBusTuple>), HipError> {
        let airs = self.segment_airs(ctx);
        let mut summaries = vec![ffi::PwBusSummary::default(); if bus_ids.is_empty() { 4096 } else { bus_ids.len() }];
        let mut tuples = vec![ffi::PwBusTuple::default(); tuple_cap];
        let (mut n_summaries, mut n_tuples) = (0usize, 0usize);
        HipError::from_result(unsafe {
            ffi::pw_check_segment_buses(airs.as_ptr(), airs.len(), bus_ids.as_ptr(), bus_ids.len(), 0, 0, 0, summaries.as_mut_ptr(),
                                        summaries.len(), &mut n_summaries,
                                        if tuple_cap == 0 { core::ptr::null_mut() } else { tuples.as_mut_ptr() }, tuple_cap, &mut n_tuples)
        })?;
        summaries.truncate(n_summaries);
        tuples.truncate(n_tuples);
        Ok((summaries, tuples))
    }

    /// The memory boundary AIR's trace from what the AIRs of `ctx` put on the memory bus, into `d_trace_out`
    /// (18 x 2^cap_log_height words on the device): `(status, log_height, touched locations)`, status 0 = written. The caller adds
    /// the AIR to the context and runs `debug_segment_buses` on the bus: this call pairs first and last accesses, it proves nothing.
    pub fn memory_boundary_trace(&self, ctx: &ProvingContext<HipBackend>, memory_bus: u32, d_trace_out: *mut u32, cap_log_height: u32)
                                 -> Result<(u32, u32, u64), HipError> {
        let airs = self.segment_airs(ctx);
        let (mut log_height, mut status, mut n_locations) = (0u32, 0u32, 0u64);
        HipError::from_result(unsafe {
            ffi::pw_memory_boundary_trace(airs.as_ptr(), airs.len(), memory_bus, 0, d_trace_out, cap_log_height, &mut log_height, &mut n_locations,
                                          &mut status)
        })?;
        Ok((status, log_height, n_locations))
    }

    /// The CPU verification step (`verify_app_proof::<BabyBearPoseidon2CpuEngine>`, openvm-riscv/src/lib.rs:337-341)
    pub fn verify_segment(&self, programs: &[AirProgram], proof: &HipSegmentProof) -> Result<(), i32> {
        let descs: Vec<ffi::PwAirDescription> = proof
            .air_ids
            .iter()
            .zip(&proof.log_heights)
            .map(|(id, lh)| {
                let p = &programs[*id];
                ffi::PwAirDescription {
                    width: p.width, log_height: *lh, logup: 1,
                    cons_bytecode: p.cons_bytecode.as_ptr(), bytecode_len: p.cons_bytecode.len(),
                    cons_spans: p.cons_spans.as_ptr(), n_constraints: p.cons_spans.len() / 2,
                    interactions: p.interactions.as_ptr(), n_interactions: p.interactions.len() / 3,
                    inter_spans: p.inter_spans.as_ptr(), n_inter_spans: p.inter_spans.len() / 2,
                    inter_bytecode: p.inter_bytecode.as_ptr(), inter_bytecode_len: p.inter_bytecode.len(),
                }
            })
            .collect();
        let mut total = [0u32; 4];
        // (the public-values verifier: exactly pw_verify_segment for segments without a row-aware AIR or public values; the values the
        // proof carries are accepted here — `pw_segment_proof_public_values` reads them, `pw_verify_segment_chain` links segments)
        let publics: Vec<ffi::PwAirPublic> =
            proof.air_ids.iter().map(|id| ffi::PwAirPublic { n: programs[*id].n_public, expected: core::ptr::null() }).collect();
        let rc = unsafe {
            ffi::pw_verify_segment_public(&self.config, descs.as_ptr(), core::ptr::null(), publics.as_ptr(), descs.len(), 1, proof.words.as_ptr(),
                                          proof.words.len(), 1, total.as_mut_ptr())
        };
        if rc == 0 { Ok(()) } else { Err(rc) }
    }
}

/// Constraint programs + interaction tables of one AIR (host memory), the keygen output the engine needs.
pub struct AirProgram {
    pub width: u32,
    pub cons_bytecode: Vec<u32>,
    pub cons_spans: Vec<u32>,     // {off, len} pairs
    pub interactions: Vec<u32>,   // {bus, n_args, first span} triples
    pub inter_spans: Vec<u32>,    // {off, len} pairs, [mult, arg0, ...] per interaction
    pub inter_bytecode: Vec<u32>,
    /// `BaseAirWithPublicValues::num_public_values`: constraint operands 2 * width + 3 + k; 0 for `PowdrAir`
    pub n_public: u32,
}

impl AirProgram {
    /// a constraint operand at or beyond `width`: a next-row column or a row selector
    pub fn reads_rows(&self) -> bool {
        self.cons_spans.chunks(2).any(|sp| {
            let code = &self.cons_bytecode[sp[0] as usize..(sp[0] + sp[1]) as usize];
            let mut ip = 0;
            while ip < code.len() {
                let op = code[ip];
                ip += 1;
                if op == 0 || op == 1 {
                    // PUSH_APC / PUSH_CONST and their operand
                    if op == 0 && ip < code.len() && code[ip] >= self.width && code[ip] < 2 * self.width + 3 {
                        return true;
                    }
                    ip += 1;
                }
            }
            false
        })
    }
}

impl StarkEngine for HipEngine {
    type SC = BabyBearSC;
    type PB = HipBackend;
    type PD = HipDevice;
    // (EXTERNAL trait) fn prove(&self, pk: &MultiStarkProvingKey<Self::SC>, ctx: ProvingContext<Self::PB>) -> Proof<Self::SC>
    //   => self.prove_segment(&ctx), wrapped into the proof type the SDK serialises
}

/// `ProverDevice`: uploads host matrices for chips that still generate traces on the CPU (system chips)
pub struct HipDevice;
impl HipDevice {
    pub fn transport_matrix_to_device(&self, values: &[BabyBear], height: usize, width: usize) -> DeviceMatrix<BabyBear> {
        // row-major host matrix -> column-major device matrix
        let mut cm = vec![values[0]; values.len()];
        for r in 0..height {
            for c in 0..width {
                cm[c * height + r] = values[r * width + c];
            }
        }
        let m = DeviceMatrix::<BabyBear>::with_capacity(height, width);
        let staged: DeviceBuffer<BabyBear> = cm.as_slice().to_device().expect("H2D");
        // (a device-to-device copy into `m`; elided: DeviceMatrix::from_buffer in a full implementation)
        let _ = staged;
        m
    }
}

// ---------------------------------------------------------------------------------------------------------------------
/// lib.rs:133-166 with the HIP engine
#[derive(Default, Clone)]
pub struct SpecializedConfigHipBuilder<ISA> {
    _marker: PhantomData<ISA>,
}

impl<ISA: OpenVmIsaHip> VmBuilder<HipEngine> for SpecializedConfigHipBuilder<ISA> {
    type VmConfig = SpecializedConfig<ISA>;
    type SystemChipInventory = <<ISA as OpenVmIsaHip>::HipBuilder as VmBuilder<HipEngine>>::SystemChipInventory;
    type RecordArena = DenseRecordArena;

    fn create_chip_complex(
        &self,
        config: &SpecializedConfig<ISA>,
        circuit: AirInventory<BabyBearSC>,
    ) -> Result<VmChipComplex<BabyBearSC, Self::RecordArena, HipBackend, Self::SystemChipInventory>, ChipInventoryError> {
        // `OpenVmIsaHip::HipBuilder` (src/isa_hip.rs): the instruction set's builder for this engine — the third one beside
        // `CpuBuilder` / `GpuBuilder` of `OpenVmISA` (isa.rs:63-81), which upstream does not have
        let mut chip_complex =
            VmBuilder::<HipEngine>::create_chip_complex(&<ISA as OpenVmIsaHip>::HipBuilder::default(), &config.original.config, circuit)?;
        let inventory = &mut chip_complex.inventory;
        VmProverExtension::<HipEngine, _, _>::extend_prover(&PowdrHipProverExt::<ISA>::default(), &config.powdr, inventory)?;
        Ok(chip_complex)
    }
}

/// lib.rs:202-269 with the HIP chips
#[derive(Default)]
pub struct PowdrHipProverExt<ISA> {
    _marker: PhantomData<ISA>,
}

impl<ISA: OpenVmIsaHip> VmProverExtension<HipEngine, DenseRecordArena, PowdrExtension<BabyBear, ISA>> for PowdrHipProverExt<ISA> {
    fn extend_prover(
        &self,
        extension: &PowdrExtension<BabyBear, ISA>,
        inventory: &mut ChipInventory<BabyBearSC, DenseRecordArena, HipBackend>,
    ) -> Result<(), ChipInventoryError> {
        // the three shared periphery chips and their bus ids, read from the AIR inventory like lib.rs:337-364
        let ids: PeripheryBusIds = powdr_openvm::get_periphery_bus_ids(inventory);
        let periphery = PowdrPeripheryInstancesHip::from_inventory(inventory, &ids);
        for precompile in &extension.precompiles {
            inventory.next_air::<PowdrAir<BabyBear>>()?;
            let chip = PowdrChipHip::new(precompile.clone(), extension.airs.clone(), extension.base_config.clone(), periphery.clone());
            inventory.add_executor_chip(chip);
        }
        Ok(())
    }
}

impl PowdrPeripheryInstancesHip {
    /// Histograms of the real and the dummy periphery instances (cuda/periphery.rs:24-85): zero-filled device buffers of
    /// `var_num_bins`, `sz0 * sz1` and `2 << 16` u32 counters.
    pub fn from_inventory<SC, RA, PB>(_inventory: &ChipInventory<SC, RA, PB>, ids: &PeripheryBusIds) -> Self {
        let alloc = |n: usize| -> *mut u32 {
            let b = DeviceBuffer::<u32>::with_capacity(n);
            b.fill_zero().expect("memset");
            let p = b.as_mut_ptr();
            core::mem::forget(b); // owned by the periphery instance for the lifetime of the VM
            p
        };
        let make = || ffi::PowdrPeriphery {
            var_range_bus_id: ids.range_checker as u32,
            d_var_hist: alloc(1 << 18),
            var_num_bins: 1 << 18,
            tuple2_bus_id: ids.tuple_range_checker.map(|x| x as u32).unwrap_or(u32::MAX),
            d_tuple2_hist: alloc(256 * 2048),
            tuple2_sz0: 256,
            tuple2_sz1: 2048,
            bitwise_bus_id: ids.bitwise_lookup.map(|x| x as u32).unwrap_or(u32::MAX),
            d_bitwise_hist: alloc(2 << 16),
        };
        Self { real: make(), dummy: make() }
    }
}
