"""tests/golden/reference_fixtures.tar.gz: the reference checkout's data fixtures that the tests read (`reference_dir` in
tests/conftest.py unpacks it once per session), under the same relative paths, so that the suite runs on a checkout of this
repository alone:
    autoprecompiles/tests/<name>.json.gz          ApcWithBusMap exports (byte for byte)
    openvm-riscv/tests/openvm_constraints.txt      the 13 RV32IM instruction AIRs as text
    openvm-riscv/tests/apc_snapshots/*/*.txt       the optimised-APC snapshots
and reference_interfaces.json: the names the Rust adapter tests pin, extracted from the reference's sources (the parameter names of
its three extern "C" functions in openvm/src/cuda_abi.rs, the members of the `OpenVmISA` trait in openvm/src/isa.rs).
    python tests/golden/make_reference_fixtures.py <reference checkout>"""
import gzip
import io
import json
import re
import sys
import tarfile
from pathlib import Path

OUT = Path(__file__).resolve().parent / "reference_fixtures.tar.gz"
APC_FIXTURES = ["single_div_nondet", "apc_reth_op_bug", "keccak_apc_pre_opt", "wasm_register_reuse"]


def interfaces(src: Path) -> dict:
    abi = (src / "openvm" / "src" / "cuda_abi.rs").read_text()
    block = abi[abi.index('extern "C"'):abi.index("#[repr(C)]")]
    strip = lambda s: re.sub(r"//[^\n]*", "", s)
    fns = {m.group(1): re.findall(r"(\w+)\s*:", strip(m.group(2))) for m in re.finditer(r"pub fn (\w+)\s*\((.*?)\)\s*->", block, flags=re.S)}
    isa = (src / "openvm" / "src" / "isa.rs").read_text()
    trait = isa[isa.index("pub trait OpenVmISA"):]
    members = sorted(set(re.findall(r"\bfn (\w+)", trait)) | set(re.findall(r"\btype (\w+)", trait)))
    return {"cuda_abi_extern_c_params": fns, "openvm_isa_members": members}


def main(src: Path):
    files = {f"autoprecompiles/tests/{n}.json.gz": (src / "autoprecompiles/tests" / f"{n}.json.gz").read_bytes() for n in APC_FIXTURES}
    files["openvm-riscv/tests/openvm_constraints.txt"] = (src / "openvm-riscv/tests/openvm_constraints.txt").read_bytes()
    for f in sorted((src / "openvm-riscv/tests/apc_snapshots").glob("*/*.txt")):
        files[f"openvm-riscv/tests/apc_snapshots/{f.parent.name}/{f.name}"] = f.read_bytes()
    files["reference_interfaces.json"] = (json.dumps(interfaces(src), sort_keys=True) + "\n").encode()
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.PAX_FORMAT) as tar:  # same bytes from the same inputs: no times, owners
        for name in sorted(files):
            info = tarfile.TarInfo(name)
            info.size, info.mode = len(files[name]), 0o644
            tar.addfile(info, io.BytesIO(files[name]))
    OUT.write_bytes(gzip.compress(buf.getvalue(), mtime=0))


if __name__ == "__main__":
    main(Path(sys.argv[1]))
