"""The directory is the list: every .hip and .cpp directly under surtr_amd/csrc is a translation unit of the library and every .h
there is a dependency of it.  The product build names its units one by one (__graft_entry__.SOURCES); tests/emul/Makefile and
scripts/build_stamp.sh take them from the directory.  These two tests keep the three from drifting apart: a unit left out of the
explicit list, or one that an emulation variant does not hold, shows here and not as an entry point missing in some later test."""
import ctypes
import glob
import os
import re

import pytest

import __graft_entry__ as G

VARIANTS = ("libsurtr_emul.so", "libsurtr_emul_small.so", "libsurtr_emul_mid.so", "libsurtr_emul_rec.so")


def _names(*patterns):
    return sorted(os.path.basename(p) for pat in patterns for p in glob.glob(os.path.join(G.CSRC, pat)))


def test_the_build_compiles_the_directory(monkeypatch):
    assert sorted(G.SOURCES) == _names("*.hip", "*.cpp")

    class Seen(Exception):
        pass

    def newer(target, deps):        # what build() hands to its up-to-date check; nothing is built
        raise Seen(deps)

    monkeypatch.setattr(G, "_newer", newer)
    with pytest.raises(Seen) as e:
        G.build()
    deps = set(e.value.args[0])
    headers = _names("*.h")
    assert headers
    for h in headers:
        assert os.path.join(G.CSRC, h) in deps, h
    assert os.path.join(G.ROOT, "include", "surtr_hip.h") in deps


def test_every_declared_function_is_in_every_emulation_variant(emul_lib_path):
    header = open(os.path.join(G.ROOT, "include", "surtr_hip.h")).read()
    names = sorted(set(re.findall(r"\b(surtr_[a-z0-9_]+)\s*\(", header)))
    assert names
    for variant in VARIANTS:
        lib = ctypes.CDLL(os.path.join(os.path.dirname(emul_lib_path), variant))
        missing = [n for n in names if not hasattr(lib, n)]
        assert not missing, (variant, missing)
