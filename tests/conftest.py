import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

# the reference checkout's data fixtures the tests read, under their paths there (tests/golden/make_reference_fixtures.py)
REFERENCE_FIXTURES = ROOT / "tests" / "golden" / "reference_fixtures.tar.gz"

# the test suite keeps the specialised kernels' code objects under the system temporary directory instead of ~/.cache/powdr_jit
# (the product's default): nothing outside the repository and /tmp is written by running the tests
import os  # noqa: E402
import tempfile  # noqa: E402

# ... in a per-user directory that only this user can write to (the library refuses any other kind: code objects are loaded from it)
_jit_cache = Path(tempfile.gettempdir()) / f"powdr_jit_cache_{os.getuid()}"
try:
    _jit_cache.mkdir(mode=0o700, exist_ok=True)
except OSError:
    pass
os.environ.setdefault("POWDR_JIT_CACHE_DIR", str(_jit_cache))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: a parametrisation whose statement a cheaper one of the same test already makes; runs with POWDR_RUN_SLOW=1 "
                                       "(the driver's `pytest -m gpu` stays under 480 s: VERDICT r5 #6)")
    # The product has no CPU fallback: make sure the HIP library (and the oracle, the checker) exist.
    # hipcc cross-compiles gfx950 without a GPU; this is a no-op when everything is up to date.
    from powdr_amd import build as _build

    _build.build()
    from oracle import apc_model as _om

    _om.build_c_oracle()


@pytest.fixture(scope="session")
def reference_dir(tmp_path_factory):
    """REFERENCE_FIXTURES unpacked once per session into a temporary directory (regular files under relative paths only)."""
    import tarfile

    out = tmp_path_factory.mktemp("reference")
    with tarfile.open(REFERENCE_FIXTURES) as tar:
        for m in tar.getmembers():
            assert m.isfile() and not m.name.startswith("/") and ".." not in Path(m.name).parts, m.name
            dst = out / m.name
            dst.parent.mkdir(parents=True, exist_ok=True)
            dst.write_bytes(tar.extractfile(m).read())
    return out


def pytest_collection_modifyitems(config, items):
    if os.environ.get("POWDR_RUN_SLOW"):
        return
    skip = pytest.mark.skip(reason="slow parametrisation (POWDR_RUN_SLOW=1 runs it); its cheaper sibling makes the same statement")
    for item in items:
        if "slow" in item.keywords:
            item.add_marker(skip)
