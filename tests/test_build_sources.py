"""CPU: the two build paths compile the same sources.  The top-level Makefile (`make lib`, for a C host) and
synth_tools_amd/build.py (`build()`) each list the library's sources; a file missing from one list links there
but leaves an undefined symbol that only shows when the library is loaded."""
import os
import re

from synth_tools_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_srcs(text):
    """The words of the Makefile's `SRCS := ...` assignment, continuation lines included."""
    m = re.search(r"^SRCS\s*:?=((?:[^\n]*\\\n)*[^\n]*)", text, re.M)
    assert m, "no SRCS assignment in the Makefile"
    return m.group(1).replace("\\\n", " ").split()


def test_makefile_lists_the_build_sources():
    with open(os.path.join(ROOT, "Makefile")) as f:
        srcs = makefile_srcs(f.read())
    assert len(srcs) == len(set(srcs))
    assert sorted(srcs) == sorted(build.SOURCES)


def test_makefile_srcs_parser():
    text = "CSRC := x\nSRCS    := a.hip b.hip \\\n           c.cpp\nOBJS := $(SRCS)\n"
    assert makefile_srcs(text) == ["a.hip", "b.hip", "c.cpp"]
