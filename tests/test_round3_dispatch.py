"""The decision-table entries of the batched round 3, append and set-values calls (include/mrbf.h: MRBF_ENTRY_DB_ROUND3 = 17,
MRBF_ENTRY_DB_APPEND_BATCH = 18, MRBF_ENTRY_DB_SET_VALUES_BATCH = 19; -2, and only -2, means "do it on the host") and the size of
their job structs as ctypes sees them against the header's static_asserts (112, 48 and 40 bytes).  No GPU."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import morbit.jl_amd as pkg

    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return pkg._lib.load()


def test_entry_numbers_match_the_header():
    from morbit.jl_amd import _lib

    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    for name, value in (("DB_ROUND3", 17), ("DB_APPEND_BATCH", 18), ("DB_SET_VALUES_BATCH", 19)):
        assert re.search(r"MRBF_ENTRY_%s = %d\b" % (name, value), text), name
        assert getattr(_lib, "ENTRY_" + name) == value
    assert (_lib.R3_UPDATE, _lib.R3_IMPROVE, _lib.R3_DONE, _lib.R3_REBUILT) == (0, 1, 0, 1)
    assert re.search(r"MRBF_R3_UPDATE = 0, MRBF_R3_IMPROVE = 1", text) and re.search(r"MRBF_R3_DONE = 0, MRBF_R3_REBUILT = 1", text)


def test_only_minus_two_means_host(lib):
    for entry in (17, 18, 19):
        for rc in range(-12, 12):                      # invalid arguments (-1 ..), MRBF_OK, the library's own error codes (1 ..)
            assert lib.mrbf_dispatch_after(entry, rc) == (1 if rc == -2 else 0), (entry, rc)


def test_the_calls_are_routed_by_the_database_rule(lib):
    assert lib.mrbf_dispatch_db_batch(1, 1) == 1 and lib.mrbf_dispatch_db_batch(65535, 4096) == 1
    assert lib.mrbf_dispatch_db_batch(0, 3) == 0 and lib.mrbf_dispatch_db_batch(65536, 3) == 0 and lib.mrbf_dispatch_db_batch(4, 4097) == 0


def test_job_struct_sizes():
    from morbit.jl_amd import _lib

    assert ctypes.sizeof(_lib.Round3Job) == 112 and _lib.Round3Job.new_sites_out.offset == 80 and _lib.Round3Job.n_new.offset == 96
    assert ctypes.sizeof(_lib.DbAppendJob) == 48 and _lib.DbAppendJob.first_index.offset == 32
    assert ctypes.sizeof(_lib.DbSetValuesJob) == 40 and _lib.DbSetValuesJob.rc.offset == 32
    text = open(os.path.join(ROOT, "include", "mrbf.h")).read()
    for name, size in (("mrbf_round3_job", 112), ("mrbf_db_append_job", 48), ("mrbf_db_set_values_job", 40)):
        assert re.search(r"\} %s;\s*/\* %d bytes \*/" % (name, size), text), name
