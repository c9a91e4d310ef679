"""The retired m_func forms (ops/linalg.py, csrc/s4.hip): an environment variable that selects
a removed arm is refused at import, and a removed pass mode is refused by the oracle and by
the library."""
import os
import subprocess
import sys

import pytest
import torch

# variable -> (the value that selected the removed arm, the harmless value)
RETIRED = {"PFML_SPD_SYM": ("0", "1"), "PFML_DB_SYM": ("0", "1"), "PFML_DB_SYMPROD": ("0", "1"),
           "PFML_M0_CANCEL": ("0", "1"), "PFML_SPD_NODE": ("0", "1"),
           "PFML_DB_NS_TAIL": ("0", "1"), "PFML_SYM_GEMM_CFG": ("2", "0")}


def test_retired_variables_refused_at_import():
    """Each retired variable at its removed value makes ``import pfml.ops.linalg`` raise a
    ValueError naming the variable and saying it is retired; at its harmless value the import
    succeeds.  The variables are read at import, so a child process reloads the module under
    each setting (a reload here would replace the module the other tests hold)."""
    code = ("import importlib, os, re\n"
            f"retired = {RETIRED!r}\n"
            "for k in retired:\n"
            "    os.environ.pop(k, None)\n"
            "from pfml.ops import linalg\n"
            "out = []\n"
            "for k, (gone, ok) in retired.items():\n"
            "    os.environ[k] = gone\n"
            "    try:\n"
            "        importlib.reload(linalg)\n"
            "        out.append(k + ' not refused')\n"
            "    except ValueError as e:\n"
            "        if not re.search(k + '.*retired', str(e)):\n"
            "            out.append(k + ' message: ' + str(e))\n"
            "    os.environ[k] = ok\n"
            "    importlib.reload(linalg)\n"
            "    del os.environ[k]\n"
            "print(out)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "[]"


def test_mf_sym_unknown_mode_cpu():
    """Mode 3 (the former sigma_hat pass) left with its code: the oracle has no catch-all."""
    from pfml.ops.linalg import mf_sym
    X = torch.eye(5, dtype=torch.float64).repeat(2, 1, 1)
    for mode in (3, 5, -1):
        with pytest.raises(ValueError, match="mode"):
            mf_sym(mode, X, X.clone(), torch.empty_like(X), d=2.0)


@pytest.mark.gpu
def test_retired_mf_mode_refused(gpu):
    """pfml_mfunc_sym's mode 3 is an invalid value: nothing is queued, out keeps its
    sentinel."""
    import ctypes as C
    from pfml.ops import _native as nat, linalg as la
    B, N = 2, 37
    X = torch.ones((B, N, N), dtype=torch.float64, device=gpu)
    Y = torch.ones_like(X)
    out = torch.full_like(X, -7.25)
    for mode in (3, 5):
        args = la._MfArgs(mode, B, N, N, N * N, X.data_ptr(), Y.data_ptr(), out.data_ptr(),
                          None, None, None, None, 0, 2.0, 0)
        with pytest.raises(RuntimeError, match="pfml_mfunc_sym failed with hipError 1"):
            nat.check(nat.hip_lib().pfml_mfunc_sym(C.byref(args), nat.stream_of(X)),
                      "pfml_mfunc_sym")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((B, N, N), -7.25, dtype=torch.float64))
