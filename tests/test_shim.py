"""The DuckDB extension shim (duckdb-cubit_amd/shim/cubit_extension.cpp) type-checks against
the reference's own DuckDB v1.1.2 headers: every DuckDB API it uses exists with the
signature it assumes. Needs the reference source tree (this container only); skipped
elsewhere. Nothing is built or linked from the reference."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import ROOT

DUCKDB_INCLUDE = Path("/root/reference/src/include")
if os.environ.get("DUCKDB_INCLUDE"):  # the Makefile's variable: a DuckDB v1.1.2 tree's src/include
    DUCKDB_INCLUDE = Path(os.environ["DUCKDB_INCLUDE"])


def _headers_readable() -> bool:
    """The headers are a file tree outside the repository: absent or unreadable (another user's
    directory) both mean the check cannot run here."""
    try:
        with open(DUCKDB_INCLUDE / "duckdb.hpp", "rb"):
            return True
    except OSError:
        return False


def test_shim_compiles_against_duckdb_headers():
    if not _headers_readable():
        pytest.skip("needs the DuckDB v1.1.2 headers (DUCKDB_INCLUDE), none readable on this machine")
    if shutil.which("g++") is None:
        pytest.skip("needs g++, not found")
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "duckdb-cubit_amd"), "shim-check",
                        f"DUCKDB_INCLUDE={DUCKDB_INCLUDE}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
