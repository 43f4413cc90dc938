"""Shared test plumbing: adapters that let the numpy oracle call the 2D networks (plain torch modules
of the product package, run on CPU), small comparison utilities, the binding switch of the GPU suites and the
C-compiler check of the ctypes descriptor mirrors."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


from oracle.nets2d import Nets2D, sd_numpy  # noqa: F401  (shared with bench.py's cpu_baseline leg)


def checksum(a):
    a = np.asarray(a, np.float64).reshape(-1)
    idx = torch.linspace(0, a.size - 1, 64).long().numpy()      # identical to tools/gen_golden.py
    return np.concatenate([[a.sum(), np.abs(a).sum()], a[idx]])


def err_stats(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(d.max()), float(d.mean())


def checksum_close(a, ref, tol=2e-4):
    """sum / abs-sum compared relatively, the 64 sampled voxels absolutely."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    rel = np.abs(a[:2] - ref[:2]) / np.maximum(np.abs(ref[:2]), 1.0)
    return bool(rel.max() < 1e-5 and np.abs(a[2:] - ref[2:]).max() < tol)


def _binding(monkeypatch, name):
    """run the rest of the test under the binding ``name`` ("torch" / "ctypes"); the operator library is loaded first either way"""
    from estdepth_amd import ops
    ops.T()
    monkeypatch.setattr(ops, "BINDING", name)


def check_desc_layout(tmp_path, struct, mirror, renamed=None, macros=()):
    """sizeof / offsetof of ``struct`` (include/estd_hip.h) as the C compiler sees it == the ctypes ``mirror``; ``renamed`` maps a mirror
    field to its C member (in_ -> in).  Returns the values of the ESTD_* ``macros`` as the header defines them."""
    fields = [f[0] for f in mirror._fields_]
    lines = ['printf("%%zu\\n", sizeof(%s));' % struct]
    lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (struct, (renamed or {}).get(f, f)) for f in fields]
    lines += ['printf("%%lld\\n", (long long)(%s));' % m for m in macros]
    src = tmp_path / ("layout_%s.c" % struct)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "estd_hip.h"\nint main(){\n' + "\n".join(lines) + "\nreturn 0;}\n")
    exe = tmp_path / ("layout_%s" % struct)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert len(out) == 1 + len(fields) + len(macros)
    assert out[0] == ctypes.sizeof(mirror)
    for f, off in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == off, f
    return out[1 + len(fields):]
