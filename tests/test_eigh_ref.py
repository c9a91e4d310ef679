"""The sequential numpy model of the device eigensolver (tests/jacobi_ref.py) against LAPACK,
its pair schedule, and the CPU branches of ``eigh_psd`` / ``m_tilde0_eig``.  The model's
figures at these sizes and at N = 496 are recorded in profiles/r12_eigh_jacobi.md; the bounds
of tests/test_gpu_eigh.py rest on them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jacobi_ref as jr

# in the model's units (N u |A|_2, N u, N u |A|_2): the bounds first set for the device solver,
# which the model itself keeps at these sizes with room (profiles/r12_eigh_jacobi.md)
RESID_MAX, ORTH_MAX, EIG_MAX = 4.0, 8.0, 4.0


@pytest.mark.parametrize("N", [1, 2, 7, 8, 17, 40, 129, 577, 1152])
def test_schedule_visits_every_pair_once(N):
    pairs = list(jr.sweep_pairs(N))
    assert len(pairs) == N * (N - 1) // 2
    assert len(set(pairs)) == len(pairs)
    assert all(0 <= p < q < N for p, q in pairs)


def test_inner_rounds_are_disjoint():
    """The pairs a workgroup runs at once (one per wave) share no column."""
    for w in (4, 8):
        m = 2 * w
        for ir in range(m - 1):
            cols = [c for k in range(w) for c in jr.tournament(m, ir, k)]
            assert sorted(cols) == list(range(m))
        for ir in range(w):
            cols = [c for k in range(w) for c in (k, w + (k + ir) % w)]
            assert sorted(cols) == list(range(m))


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("N", [1, 2, 7, 17, 40, 100])
def test_model_matches_lapack(N, which):
    A = jr.spectra(N)[which]
    e, Vt, sweeps, conv = jr.jacobi_eigh(A)
    f = jr.figures(A, e, Vt)
    print(f"N = {N} spectrum {which}: sweeps {sweeps} resid {f['resid']:.3f} "
          f"orth {f['orth']:.3f} eig {f['eig']:.3f}")
    assert conv and sweeps <= 30
    assert f["resid"] <= RESID_MAX and f["orth"] <= ORTH_MAX and f["eig"] <= EIG_MAX


def test_repair_switch_is_read_from_the_environment():
    """PFML_MFUNC_REPAIR_EIG: unset and "1" take the device root, "0" the host root.  The
    module constant is read at import, so a child process reloads the module under each
    value (a reload here would replace the module the other tests hold)."""
    code = ("import importlib, os\n"
            "from pfml.ops import linalg\n"
            "out = []\n"
            "for v in (None, '1', '0', ''):\n"
            "    os.environ.pop('PFML_MFUNC_REPAIR_EIG', None)\n"
            "    if v is not None:\n"
            "        os.environ['PFML_MFUNC_REPAIR_EIG'] = v\n"
            "    out.append(importlib.reload(linalg).MFUNC_REPAIR_EIG)\n"
            "print(out)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "[True, True, False, True]"


def test_eigh_psd_cpu_layout():
    """CPU tensors: torch.linalg.eigh in the device layout (rows of Vt are eigenvectors)."""
    from pfml.ops.linalg import eigh_psd
    A = torch.tensor(np.stack(jr.spectra(17)))
    A0 = A.clone()
    e, Vt = eigh_psd(A)
    assert e.shape == (3, 17) and Vt.shape == (3, 17, 17) and torch.equal(A, A0)
    rec = Vt.transpose(1, 2) @ torch.diag_embed(e) @ Vt
    for b in range(3):
        assert (rec[b] - A[b]).abs().max() <= 1e-13 * A[b].abs().max()
    with pytest.raises(ValueError):
        eigh_psd(torch.zeros(3, 4, 5, dtype=torch.float64))


def test_m_tilde0_eig_cpu_solves_its_quadratic():
    """m0 (x + 2I) - m0^2 - I = 0, m0 exactly symmetric (the CPU branch)."""
    from pfml.ops.linalg import m_tilde0_eig
    x = torch.tensor(np.stack(jr.spectra(40)))
    m0 = m_tilde0_eig(x)
    assert torch.equal(m0, m0.transpose(1, 2))
    I = torch.eye(40, dtype=torch.float64)
    assert (m0 @ (x + 2.0 * I) - m0 @ m0 - I).abs().max().item() <= 1e-11
