"""tw_set_trace_batch's public surface, without a GPU: the header declares it
with the documented signature and the Python engine exposes it (test_abi.py
checks that the library exports every declared symbol)."""
import inspect
import os
import re

from timewarp import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "timewarp.h")


def test_header_declares_tw_set_trace_batch():
    src = open(HEADER).read()
    assert re.search(r"^int\s+tw_set_trace_batch\(\s*tw_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", src, re.M)
    assert "tw_set_trace_batch" in engine.EXPORTS


def test_engine_has_set_trace_batch():
    sig = inspect.signature(engine.Engine.set_trace_batch)
    assert list(sig.parameters) == ["self", "on"]
    assert engine.LPEngine.set_trace_batch is engine.Engine.set_trace_batch   # (answers ERR_INVALID there)
    assert "set_trace_batch" in engine.Engine.set_trace.__doc__
