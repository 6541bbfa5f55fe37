"""The decision-table rows of the resident site database (csrc/dispatch.hip, include/mrbf.h "decision table") pinned at their boundaries
without a GPU: mrbf_dispatch_db_batch answers device for 1 <= n_starts <= 65535 and 1 <= d <= 4096, and for MRBF_ENTRY_DB_BOX /
MRBF_ENTRY_DB_GATHER a return code of -2 -- and only that -- means "do it on the host"."""
import ctypes
import os

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


@pytest.mark.parametrize("n_starts,d,device", [(0, 1, 0), (1, 1, 1), (65535, 1, 1), (65536, 1, 0), (1, 0, 0), (1, 4096, 1), (1, 4097, 0),
                                               (65535, 4096, 1), (0, 4097, 0), (-1, 3, 0), (3, -1, 0), (64, 128, 1)])
def test_db_batch_boundaries(lib, n_starts, d, device):
    from morbit.jl_amd import _lib

    assert lib.mrbf_dispatch_db_batch(n_starts, d) == (_lib.DISPATCH_DEVICE if device else _lib.DISPATCH_REFERENCE)


def test_db_entries_fall_back_on_minus_two_only(lib):
    from morbit.jl_amd import _lib

    assert (_lib.ENTRY_DB_BOX, _lib.ENTRY_DB_GATHER) == (15, 16)
    for entry in (_lib.ENTRY_DB_BOX, _lib.ENTRY_DB_GATHER):
        assert lib.mrbf_dispatch_after(entry, -2) == 1
        for rc in (0, -1, -3, -4, -5, _lib.MRBF_ESINGULAR, _lib.MRBF_EHIP, _lib.MRBF_ENOMEM):
            assert lib.mrbf_dispatch_after(entry, rc) == 0, (entry, rc)


def test_db_job_layouts_match_header():
    from morbit.jl_amd import _lib

    assert ctypes.sizeof(_lib.DbBoxJob) == 120 and _lib.DbBoxJob.rc.offset == 52 and _lib.DbBoxJob.mc.offset == 88
    assert ctypes.sizeof(_lib.DbGatherJob) == 64 and _lib.DbGatherJob.rc.offset == 56
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    assert "MRBF_ENTRY_DB_BOX = 15, MRBF_ENTRY_DB_GATHER = 16" in text
