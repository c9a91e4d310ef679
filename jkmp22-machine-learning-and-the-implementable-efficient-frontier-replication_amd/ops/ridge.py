"""Hyper-parameter grid kernels: ridge solves (K15) and utilities (K16); the window sums
(K14) are ops/wsum.py.

Device paths run csrc/ridge.hip and csrc/quadform.hip; CPU paths are the fp64 oracle in the
reference's own formulation (np.linalg.solve per lambda, PFML_Search_Coef.py:131-133;
r'b - 1/2 b'Db per month, PFML_hp_reals.py:94).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as nat
from ._native import upload      # noqa: F401  (tools and tests spell it ridge.upload)

CELL_DTYPE = np.dtype([("src", "<i8"), ("rsrc", "<i8"), ("work", "<i8"), ("out", "<i8"),
                       ("n", "<i4"), ("_pad", "<i4"), ("scale", "<f8")])
JOB_DTYPE = np.dtype([("d_off", "<i8"), ("r_off", "<i8"), ("b_off", "<i8"), ("o_off", "<i8"),
                      ("n", "<i4"), ("ptile0", "<i4")])


class LaunchArgs(C.Structure):
    """csrc/ridge_desc.h RidgeLaunchArgs: one ridge-grid launch, options included."""
    _P, _I, _L, _B = C.c_void_p, C.c_int, C.c_int64, C.c_bool
    _fields_ = [("SD", _P), ("ldS", _L), ("Sr", _P), ("cells", _P), ("ncells", _I), ("nmax", _I),
                ("lvec", _P), ("L", _I), ("work", _P), ("beta", _P), ("ldo", _L),
                ("lu_list", _P), ("lu_count", _P), ("lu_cap", _I), ("wgmap", _P), ("nwg", _I),
                ("syncw", _P), ("n_host", _P), ("timing", _P), ("spin_max", C.c_uint),
                ("phases", _I), ("solo", _B), ("bt_wy", _B), ("bt_classes", _B)]


nat.register_hip("pfml_ridge_grid", [C.POINTER(LaunchArgs), C.c_void_p])
nat.register_hip("pfml_ridge_timing_words", [C.c_int], C.c_int64)


class _HostClock:
    """PFML_HOST_TIMING=1: print host-side section times (microseconds) to stderr;
    PFML_HOST_TIMING=sync: synchronise the device at every mark (section = wall time of the
    queued work)."""

    def __init__(self):
        import time
        v = os.environ.get("PFML_HOST_TIMING", "")
        self.on = bool(v)
        self.sync = v == "sync" and torch.cuda.is_available()
        self.time = time.perf_counter
        if self.sync:
            torch.cuda.synchronize()
        self.t = self.time()

    def __call__(self, what: str) -> None:
        if self.on:
            import sys
            if self.sync:
                torch.cuda.synchronize()
            now = self.time()
            print(f"[host] {what}: {1e6 * (now - self.t):.0f} us", file=sys.stderr)
            self.t = now


_WORK_CACHE: dict = {}


def _work_doubles(n_arr: np.ndarray, L: int) -> np.ndarray:
    lib = nat.hip_lib()
    out = np.empty(len(n_arr), dtype=np.int64)
    for n in np.unique(n_arr):
        key = (int(n), L)
        if key not in _WORK_CACHE:
            _WORK_CACHE[key] = int(lib.pfml_ridge_work_doubles(int(n), L))
        out[n_arr == n] = _WORK_CACHE[key]
    return out


COOP_KMAX = 16          # workgroups per cell of the cooperative band reduction (wgmap: 4 bits)
COOP_SYNC_WORDS = 32    # csrc/ridge_band.h COOP_SYNC (pfml_coop_sync_words): int32 sync words per cell
COOP_BIG_SHARE = 0.42   # share of the CUs the largest cells' cooperative launch gets (coop_k)
QUAD_DIRECT, QUAD_PIPE, QUAD_PIPE_REST = 3, 4, 5     # csrc/quadform.hip pfml_quadform's `form`
# K steps the longest run of a utilities launch may take: the months of every (cell, row
# tile) are cut into runs of as many months as keep the longest tile's run within this
# (``quad_plan``; profiles/r16_experiments.md)
QUAD_RUN_STEPS = 192
QUAD_SLOTS_PER_CU = 3   # utilities workgroups resident per CU (csrc/quadform.hip launch bounds)


@dataclass(frozen=True)
class Switches:
    """Every environment variable that shapes a grid-step launch, read in one place
    (``switches()``): per field the default, and the variable that selects the other A/B arm.
    The library keeps no state: the fields it acts on travel with every launch
    (``launch_opts`` -> ``LaunchArgs``), the rest shape the host-side plans.

    coop_k         ``coop_k``'s policy; PFML_COOP_K=k (not empty): k workgroups per largest cell
    coop_solo      a launch whose cells all have K = 1 on the solo kernel; PFML_COOP_SOLO=0: not
    coop_spin_max  the library's ~1 s poll bound of the cooperative waits; PFML_COOP_SPIN_MAX=n: n
    bt_classes     a back-transform instance per size class; PFML_BT_CLASSES=0: 8 waves for all
    bt_wy          n > 1024 cells on the blocked-WY MFMA back-transform; PFML_RIDGE_BT_WY=0: generic
    two_streams    the largest cells' group and the rest on two streams; PFML_RIDGE_STREAMS=1: one
    quad_direct    the pipelined utilities form; PFML_QUAD_DIRECT not empty: the direct-A form
    quad_xcd       every utilities tile of a cell on one XCD (``_xcd_order``); PFML_QUAD_XCD=0: not

    PFML_RIDGE_STREAMS means one stream at any value but empty or 2.  Retired, ValueError both:
    PFML_QUAD_DIRECT=0, PFML_QUAD_MM=2 - the removed LDS-staged forms (PFML_QUAD_MM=1: a no-op).
    """
    coop_k: int | None = None
    coop_solo: bool = True
    coop_spin_max: int = 0
    bt_classes: bool = True
    bt_wy: bool = True
    two_streams: bool = True
    quad_direct: bool = False
    quad_xcd: bool = True


def switches() -> Switches:
    """The launch switches as the environment sets them now."""
    env = os.environ.get
    if env("PFML_QUAD_DIRECT") == "0" or env("PFML_QUAD_MM") == "2":
        raise ValueError("PFML_QUAD_DIRECT=0 and PFML_QUAD_MM=2 are retired: the LDS-staged "
                         "utilities forms they selected were removed")
    return Switches(
        coop_k=int(env("PFML_COOP_K")) if env("PFML_COOP_K") else None,
        coop_solo=env("PFML_COOP_SOLO", "1") != "0",
        coop_spin_max=int(env("PFML_COOP_SPIN_MAX", "0") or 0),
        bt_classes=env("PFML_BT_CLASSES", "1") != "0",
        bt_wy=env("PFML_RIDGE_BT_WY", "1") != "0",
        two_streams=(env("PFML_RIDGE_STREAMS") or "2").strip() == "2",
        quad_direct=env("PFML_QUAD_DIRECT", "") != "",
        quad_xcd=env("PFML_QUAD_XCD", "1") != "0")


def coop_k(cell_n: np.ndarray, ncu: int, sw: Switches | None = None) -> np.ndarray:
    """Workgroups per cell of the cooperative band reduction.

    The largest-n cells of a launch are the p = 512 cells (n > 256: 32 panels, the grid step's
    critical chain); they share about COOP_BIG_SHARE of the chip's CUs, round(0.42 ncu / n_big)
    workgroups each (at least 1, at most COOP_KMAX), and every other cell gets one workgroup:
    the smaller cells' whole chain (reduction, solves, back-transform, utilities) runs on the
    rest from a second stream and must keep pace.  Measured on the one-GPU rank rehearsal
    (tools/gpu_run.sh shardk, profiles/r04_coop_k_sweep.json): the best K is 1 / 2 / 4 / 6-8 at
    W = 1 / 2 / 4 / 8 ranks (106 / 53 / 27 / 13 big cells per rank), i.e. ~106 of 256 CUs for the
    big cells whatever W - giving them all the CUs the small cells leave (K = 16 at W = 8) was
    27 % slower per rank.  The betas do not depend on K (bitwise: see band_coop_kernel), only
    the time does.  PFML_COOP_K=k (``sw.coop_k``) forces k for the largest cells."""
    sw = sw or switches()
    n = np.asarray(cell_n)
    k = np.ones(len(n), dtype=np.int64)
    if not len(n):
        return k
    big = n == n.max()
    if sw.coop_k is not None:
        kb = sw.coop_k
    elif int(n.max()) > 256:
        kb = int(round(COOP_BIG_SHARE * ncu / int(big.sum())))
    else:
        kb = 1
    k[big] = min(max(kb, 1), COOP_KMAX)
    return k


def coop_wgmap(k: np.ndarray) -> np.ndarray:
    """Block -> (cell, rank, K) codes ``cell << 8 | w << 4 | K - 1`` for cells in plan order.
    Runs of up to 8 cells with the same K are interleaved (block b and b + 8 hold ranks w and
    w + 1 of one cell: the same XCD under the observed round-robin placement - speed only)."""
    codes = []
    c = 0
    nc = len(k)
    while c < nc:
        g = 1
        while c + g < nc and g < 8 and k[c + g] == k[c]:
            g += 1
        for w in range(int(k[c])):
            for j in range(g):
                codes.append(((c + j) << 8) | (w << 4) | (int(k[c]) - 1))
        c += g
    return np.asarray(codes, dtype=np.int32)


_NCU: dict = {}


def ranks_per_device() -> int:
    """Processes of this node sharing one device (torchrun's LOCAL_WORLD_SIZE over the visible
    devices, ranks placed LOCAL_RANK mod device_count): 1 on an N-GPU node with one rank per
    GPU, W in the one-GPU multi-process rehearsal."""
    lw = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
    nd = max(1, torch.cuda.device_count())
    return max(1, -(-lw // nd))


def num_cus(dev) -> int:
    """CUs this process may count on for the cooperative reduction: the device's, split among
    the processes that share it.  A cooperative cell's K workgroups wait for each other, so
    they must be co-resident; several processes each filling the whole chip with spinning
    workgroups would starve each other (their cells time out)."""
    key = str(dev)
    if key not in _NCU:
        _NCU[key] = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    return max(1, _NCU[key] // ranks_per_device())


def ridge_plan(P: int, L: int, cell_src, cell_n, cell_scale, ncu: int = 256,
               sw: Switches | None = None) -> dict:
    """Host-side descriptors of one ridge-grid launch (CELL_DTYPE, big cells first) and the
    workgroup map of the cooperative reduction (``ncu``: the device's CUs)."""
    lib = nat.hip_lib()
    if lib.pfml_ridge_cell_desc_size() != CELL_DTYPE.itemsize:
        raise RuntimeError("CellDesc layout mismatch between python and libpfml_hip")
    if lib.pfml_ridge_launch_args_size() != C.sizeof(LaunchArgs):
        raise RuntimeError("RidgeLaunchArgs layout mismatch between python and libpfml_hip")
    if lib.pfml_coop_sync_words() != COOP_SYNC_WORDS:
        raise RuntimeError("COOP_SYNC_WORDS differs from libpfml_hip's sync words per cell")
    nc = len(cell_src)
    cell_n = np.asarray(cell_n)
    nlim = int(lib.pfml_ridge_nmax())
    if nc and int(cell_n.max()) > nlim:
        raise ValueError(f"ridge_plan: p = {int(cell_n.max()) - 1} is above the device ridge "
                         f"grid's limit of n = p + 1 <= {nlim} (p <= {nlim - 1}); the CPU path "
                         "has no limit")
    wsz = _work_doubles(cell_n, L)
    desc = np.zeros(nc, dtype=CELL_DTYPE)
    desc["src"] = np.asarray(cell_src, np.int64) * P * P
    desc["rsrc"] = np.asarray(cell_src, np.int64) * P
    desc["out"] = np.arange(nc, dtype=np.int64) * L * P
    desc["n"] = cell_n.astype(np.int32)
    desc["scale"] = np.asarray(cell_scale, np.float64)
    # big cells first: they bound the kernel's makespan
    order = np.argsort(-desc["n"], kind="stable")
    desc = desc[order]
    wsz = wsz[order]
    desc["work"] = np.concatenate([[0], np.cumsum(wsz)[:-1]])
    wgmap = coop_wgmap(coop_k(desc["n"], ncu, sw))
    # host copy of n in plan order: the back-transform's instance per size class
    n_host = np.ascontiguousarray(desc["n"], dtype=np.int32)
    return {"desc": desc, "work": int(wsz.sum()), "nmax": int(cell_n.max()), "nc": nc,
            "wgmap": wgmap, "n_host": n_host}


nat.register_hip("pfml_ridge_repair", [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
nat.register_hip("pfml_ridge_repair_work_doubles", [C.c_int], C.c_int64)
nat.register_hip("pfml_ridge_repair_work_doubles_cap", [C.c_int, C.c_int], C.c_int64)
_REPAIR_WORK: dict = {}

# device repair counts of the most recent ridge launches (int32 device scalars; read them
# only when reporting - reading forces a sync)
LAST_REPAIRS: list = []


def repair_launch(plan: dict, d_desc: torch.Tensor, SD: torch.Tensor, Sr: torch.Tensor,
                  lv: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """Queue the device repair of the NaN-marked (non-SPD) systems of one ridge launch
    (csrc/ridge_repair.hip: pivoted-LU re-solve, np.linalg.solve semantics) on the current
    stream; returns the device count of repaired systems (no host sync)."""
    P = SD.shape[-1]
    L = int(lv.numel())
    lib = nat.hip_lib()
    count = torch.zeros(1, dtype=torch.int32, device=SD.device)
    cap = plan["nc"] * L
    lst = torch.empty(cap, dtype=torch.int32, device=SD.device)
    # scratch sized by the launch's own capacity and kept per (device, size): allocated once,
    # not per launch (540 MB per tridiagonal-path launch at n = 1025)
    nwd = int(lib.pfml_ridge_repair_work_doubles_cap(plan["nmax"], cap))
    wkey = (str(SD.device), nat.stream_of(SD), nwd)     # (per stream: no sharing across streams)
    # never evicted: a HIP graph that captured a launch keeps this buffer's raw pointer (it is
    # not in the graph's private pool), so freeing it would hand the graph's scratch to other
    # tensors; one buffer per (device, stream, size) key stays bounded
    work = _REPAIR_WORK.get(wkey)
    if work is None:
        work = _REPAIR_WORK[wkey] = torch.empty(nwd, dtype=torch.float64, device=SD.device)
    nat.check(lib.pfml_ridge_repair(SD.data_ptr(), P, Sr.data_ptr(), d_desc.data_ptr(),
                                    plan["nc"], plan["nmax"], lv.data_ptr(), L, beta.data_ptr(),
                                    beta.shape[-1], lst.data_ptr(), count.data_ptr(), cap,
                                    work.data_ptr(), nat.stream_of(SD)), "pfml_ridge_repair")
    return count


def repairs_done() -> int:
    """Host read of the repair counts of the last grid launches (one sync)."""
    return int(sum(int(c.item()) for c in LAST_REPAIRS))


def band_path(plan: dict) -> bool:
    """True when the launch takes the band path (ridge_band.hip, n <= 528), whose non-SPD
    lambdas are repaired in the band domain inside the launch; the tridiagonal path
    (ridge.hip, 528 < n <= 2049, i.e. p up to 2048) leaves NaN markers for ``repair_launch``.
    The launch's largest n decides for all its cells: ``ridge_groups`` keeps the production
    entry from mixing the two kinds in one launch."""
    return plan["nmax"] <= nat.hip_lib().pfml_ridge_band_nmax()


def launch_opts(sw: Switches, spin_override: int | None = None) -> dict:
    """The option fields of ``LaunchArgs`` that the switches set.  ``spin_override``: the
    ``set_coop_spin_max`` value (None: the module's current one); non-zero, it wins over
    ``sw.coop_spin_max``.  0 means the library's default bound."""
    if spin_override is None:
        spin_override = _SPIN_OVERRIDE[0]
    return {"spin_max": int(spin_override or sw.coop_spin_max), "solo": bool(sw.coop_solo),
            "bt_wy": bool(sw.bt_wy), "bt_classes": bool(sw.bt_classes)}


def ridge_launch(plan: dict, d_desc: torch.Tensor, SD: torch.Tensor, Sr: torch.Tensor,
                 lv: torch.Tensor, beta: torch.Tensor, repair: bool = True,
                 d_wgmap: torch.Tensor | None = None,
                 sw: Switches | None = None, *, timing: torch.Tensor | None = None,
                 phases: int = 7, work: torch.Tensor | None = None) -> torch.Tensor | None:
    """Queue one ridge-grid launch; returns the device count of non-SPD systems re-solved by
    the band path's pivoted banded LU (kernel 2b, ridge_band_solve.hip), None when the launch
    has no in-band repair (``repair=False`` or the tridiagonal path).  ``d_wgmap``: the device
    copy of plan["wgmap"] (the cooperative band reduction's workgroup map).  For this launch
    only: ``timing``, an int64 device buffer of pfml_ridge_timing_words(cells) words for the
    band path's cycle counters; ``phases``, the tridiagonal path's phases to queue (bit 0
    tridiagonalisation, 1 solves, 2 back-transform), which read the earlier phases from
    ``work`` (plan["work"] doubles, default a fresh one): that of a preceding full launch."""
    sw = sw or switches()
    lib = nat.hip_lib()
    P = SD.shape[-1]
    L = int(lv.numel())
    nc = plan["nc"]
    band = band_path(plan)
    if phases != 7 and (work is None or band):
        raise ValueError("ridge_launch: a launch with phases left out needs the work tensor of "
                         "a preceding full launch (tridiagonal path only)")
    if band and d_wgmap is None:
        raise ValueError("ridge_launch: the cooperative reduction needs the device wgmap")
    if work is None:
        work = torch.empty(plan["work"], dtype=torch.float64, device=SD.device)
    elif work.dtype != torch.float64 or work.device != SD.device or work.numel() < plan["work"]:
        raise ValueError(f"ridge_launch: work must hold {plan['work']} doubles on {SD.device}")
    if timing is not None:
        tw = lib.pfml_ridge_timing_words(nc)
        if timing.dtype != torch.int64 or timing.device != SD.device or timing.numel() < tw:
            raise ValueError(f"ridge_launch: timing must hold {tw} int64 words on {SD.device}")
    args = LaunchArgs(SD=SD.data_ptr(), ldS=P, Sr=Sr.data_ptr(), cells=d_desc.data_ptr(),
                      ncells=nc, nmax=plan["nmax"], lvec=lv.data_ptr(), L=L,
                      work=work.data_ptr(), beta=beta.data_ptr(), ldo=beta.shape[-1],
                      lu_cap=nc * L,
                      # host pointer to the plan's per-cell n (read during the launch call only)
                      n_host=plan["n_host"].ctypes.data, timing=nat.ptr(timing),
                      phases=phases, **launch_opts(sw))
    count = None
    if band:
        if repair:
            count = torch.empty(1, dtype=torch.int32, device=SD.device)   # zeroed by the solve
            lst = torch.empty(nc * L, dtype=torch.int32, device=SD.device)
            args.lu_list, args.lu_count = lst.data_ptr(), count.data_ptr()
        sync = torch.empty(nc * COOP_SYNC_WORDS, dtype=torch.int32, device=SD.device)
        # every launch's sync words are kept until the next grid search starts (the big and the
        # small cells' launches run on two streams: neither may hide the other's timeouts)
        LAST_COOP_SYNC.append(sync)
        args.wgmap, args.nwg, args.syncw = d_wgmap.data_ptr(), len(plan["wgmap"]), sync.data_ptr()
    nat.check(lib.pfml_ridge_grid(C.byref(args), nat.stream_of(SD)), "pfml_ridge_grid")
    return count


# sync words of the cooperative launches since the last ``reset_coop_sync`` (one per launch;
# the error word is index 1 of every cell's COOP_SYNC_WORDS): a timed-out cell's betas are NaN
# (the back-transform poisons them) and the grid search's non-finite recovery recomputes them
LAST_COOP_SYNC: list = []


def reset_coop_sync() -> None:
    LAST_COOP_SYNC.clear()


def coop_errors() -> int:
    """Number of cells whose cooperative hand-off wait timed out, over every launch since the
    last ``reset_coop_sync`` (one host sync)."""
    if not LAST_COOP_SYNC:
        return 0
    return int(sum(int((s.view(-1, COOP_SYNC_WORDS)[:, 1] != 0).sum().item())
                   for s in LAST_COOP_SYNC))


_SPIN_OVERRIDE = [0]


def set_coop_spin_max(n: int) -> None:
    """Poll bound of the cooperative reduction's waits for later launches (tests lower it to
    force timeouts); it wins over ``PFML_COOP_SPIN_MAX`` until it is called with 0."""
    _SPIN_OVERRIDE[0] = int(n)


def ridge_grid(SD: torch.Tensor, Sr: torch.Tensor, cell_src: np.ndarray, cell_n: np.ndarray,
               cell_scale: np.ndarray, lvec: torch.Tensor, repair: bool = True) -> torch.Tensor:
    """beta[c, l, :n_c] = solve(SD[src_c][:n,:n]*scale_c + l I, Sr[src_c][:n]*scale_c).

    SD: [S, P, P] running sums, Sr: [S, P]; returns [ncells, L, P] (zero beyond n_c).
    Non-SPD systems (NaN-marked by the banded Cholesky) are re-solved on the device by a
    pivoted banded LU before the back-transform (band path) or a dense pivoted LU after it
    (tridiagonal path, ``repair_launch``), no host sync; ``repair=False`` leaves the NaNs.
    """
    S, P, _ = SD.shape
    L = int(lvec.numel())
    nc = len(cell_src)
    # (the plan first: a cell above the device limit is refused before anything is queued)
    sw = switches()
    plan = (ridge_plan(P, L, cell_src, cell_n, cell_scale, ncu=num_cus(SD.device), sw=sw)
            if nc and nat.is_device(SD) else None)
    beta = torch.zeros((nc, L, P), dtype=SD.dtype, device=SD.device)
    if nc == 0:
        return beta
    if nat.is_device(SD):
        reset_coop_sync()
        d_desc, d_wg = upload([plan["desc"], plan["wgmap"]], SD.device)
        lv = lvec.to(device=SD.device, dtype=torch.float64).contiguous()
        SDc, Src = SD.contiguous(), Sr.contiguous()
        count = ridge_launch(plan, d_desc, SDc, Src, lv, beta, repair, d_wg, sw)
        if repair:
            LAST_REPAIRS[:] = [count if count is not None
                               else repair_launch(plan, d_desc, SDc, Src, lv, beta)]
        return beta
    eye_cache = {}
    lv = lvec.to(dtype=SD.dtype)
    for c in range(nc):
        n, s = int(cell_n[c]), int(cell_src[c])
        A = SD[s, :n, :n] * float(cell_scale[c])
        r = Sr[s, :n] * float(cell_scale[c])
        if n not in eye_cache:
            eye_cache[n] = torch.eye(n, dtype=SD.dtype)
        sys_ = A.unsqueeze(0) + lv.view(-1, 1, 1) * eye_cache[n]
        sol, info = torch.linalg.solve_ex(sys_, r.unsqueeze(0).expand(L, n).unsqueeze(-1))
        sol = sol.squeeze(-1)
        sol[info != 0] = float("nan")          # singular system (reference: LinAlgError)
        beta[c, :, :n] = sol
    return beta


def repair_nonspd(beta, SD, Sr, cell_src, cell_n, cell_scale, lv) -> np.ndarray:
    """Host-side reference of the repair: re-solve the NaN-marked (cell, lambda) systems with
    torch's pivoted LU (np.linalg.solve semantics, PFML_Search_Coef.py:131-133).  The engine
    uses the device form (``repair_launch``); this one is the test oracle."""
    bad = torch.isnan(beta).any(dim=-1)
    if not bool(bad.any()):
        return np.zeros(0, dtype=np.int64)
    cells = torch.nonzero(bad.any(dim=1)).flatten().tolist()
    for c in cells:
        ls = torch.nonzero(bad[c]).flatten()
        n, s = int(cell_n[c]), int(cell_src[c])
        A = SD[s, :n, :n] * float(cell_scale[c])
        r = Sr[s, :n] * float(cell_scale[c])
        eye = torch.eye(n, dtype=A.dtype, device=A.device)
        sys_ = A.unsqueeze(0) + lv[ls].view(-1, 1, 1) * eye
        sol, info = torch.linalg.solve_ex(sys_, r.expand(len(ls), n).unsqueeze(-1))
        sol = sol.squeeze(-1)
        sol[info != 0] = float("nan")
        beta[c, ls, :n] = sol
    return np.asarray(cells, dtype=np.int64)


_SIDE: dict = {}


def _side_stream(dev: torch.device, k: int = 0) -> torch.cuda.Stream:
    """Cached secondary HIP streams per device (stream creation is not free)."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), k)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=dev)
    return _SIDE[key]


_UTIL_PLANS: dict = {}

BAND_NMAX = 528         # csrc/ridge_band.hip BNMAX (pfml_ridge_band_nmax): the band path's largest n


def ridge_groups(cell_n, band_nmax: int = BAND_NMAX) -> list:
    """Launch groups of ``ridge_utilities`` as index arrays into ``cell_n`` (pure host code, no
    native call): the largest-n cells first, then the rest.  A launch's path is picked by its
    largest n (``band_path``), so when the rest holds both tridiagonal-path cells
    (n > ``band_nmax``) and band-path cells it is split in two, the band cells last: a band
    cell is never solved on the tridiagonal path.  With at most one n above ``band_nmax`` these
    are the two groups "largest" and "rest"."""
    n = np.asarray(cell_n)
    big = n == n.max()
    rest_tri = ~big & (n > band_nmax)
    rest_band = ~big & (n <= band_nmax)
    if rest_tri.any() and rest_band.any():
        parts = (big, rest_tri, rest_band)
    else:
        parts = (big, ~big)
    return [np.nonzero(m)[0] for m in parts]


def _utilities_plan(P: int, L: int, dev, cell_src, cell_n, cell_scale, job_cell, job_month,
                    job_n, split: bool = True, sw: Switches | None = None) -> dict:
    """Launch plan of ridge_utilities on a device, cached: the descriptors depend only on the
    grid's shape (cells, jobs, P, L) and the switches, so repeated grid searches (every step of
    a run, every benchmark step) reuse the uploaded device copies and skip all host planning.
    Each group's cells / jobs write straight into the full beta / obj arrays (global offsets)."""
    sw = sw or switches()
    key = (sw, P, L, str(dev), split,
           cell_src.tobytes(), cell_n.tobytes(), cell_scale.tobytes(),
           job_cell.tobytes(), job_month.tobytes(), job_n.tobytes())
    hit = _UTIL_PLANS.get(key)
    if hit is not None:
        return hit
    if split:
        # the largest cells (their own cooperative launch: the chip's CUs shared among them)
        # and the rest (one workgroup each; band and tridiagonal cells apart), each group on a
        # stream of its own
        if nat.hip_lib().pfml_ridge_band_nmax() != BAND_NMAX:
            raise RuntimeError("BAND_NMAX differs from libpfml_hip's band limit")
        parts = ridge_groups(cell_n)
    else:
        parts = [np.arange(len(cell_n))]
    groups, arrays = [], []
    for cells in parts:
        grp = np.zeros(len(cell_n), dtype=bool)
        grp[cells] = True
        jobs = np.nonzero(grp[job_cell])[0]
        rp = ridge_plan(P, L, cell_src[cells], cell_n[cells], cell_scale[cells], num_cus(dev), sw)
        # ridge_plan orders cells big-first and numbers outputs 0..: map to global rows
        rp["desc"]["out"] = cells[rp["desc"]["out"] // (L * P)].astype(np.int64) * L * P
        qp = quad_plan(P, L, P, job_cell[jobs], job_month[jobs], job_n[jobs], job_out=jobs, sw=sw,
                       run_steps=QUAD_RUN_STEPS, slots=QUAD_SLOTS_PER_CU * num_cus(dev))
        groups.append((cells, jobs, rp, qp))
        arrays += [rp["desc"], qp["desc"], quad_tables(qp), rp["wgmap"]]
    dv = upload(arrays, dev)                     # all descriptors, one async copy
    plan = {"groups": groups, "dv": dv}
    if len(_UTIL_PLANS) > 64:
        _UTIL_PLANS.clear()
    _UTIL_PLANS[key] = plan
    return plan


def check_launch_bounds(S: int, P: int, T: int, cell_src, cell_n, job_cell, job_month,
                        job_n) -> None:
    """Host-side guard before any ridge / utilities kernel sees the plan: every index the
    descriptors turn into a device address must be in range (a bad plan would otherwise be a
    GPU memory fault, not an exception)."""
    nc = len(cell_src)
    bad = []
    if nc and (int(np.min(cell_src)) < 0 or int(np.max(cell_src)) >= S):
        bad.append(f"cell_src outside [0, {S})")
    if nc and (int(np.min(cell_n)) < 1 or int(np.max(cell_n)) > P):
        bad.append(f"cell_n outside [1, {P}]")
    if len(job_cell):
        if int(np.min(job_cell)) < 0 or int(np.max(job_cell)) >= nc:
            bad.append(f"job_cell outside [0, {nc})")
        if int(np.min(job_month)) < 0 or int(np.max(job_month)) >= T:
            bad.append(f"job_month outside [0, {T})")
        if int(np.min(job_n)) < 1 or int(np.max(job_n)) > P:
            bad.append(f"job_n outside [1, {P}]")
    if bad:
        raise ValueError("ridge_utilities: invalid launch plan: " + "; ".join(bad))


def ridge_utilities(SD: torch.Tensor, Sr: torch.Tensor, cell_src, cell_n, cell_scale,
                    lvec: torch.Tensor, D: torch.Tensor, R: torch.Tensor, job_cell, job_month,
                    job_n) -> tuple[torch.Tensor, torch.Tensor]:
    """(beta, obj) = (ridge_grid(...), quadform_utilities(D, R, beta, jobs)).

    On a device the cells split into the largest-n group and the rest (``ridge_groups``: the
    rest in two groups when it mixes band and tridiagonal cells); each group's ridge ->
    utilities chain is issued on its own HIP stream, the big group first, so the small cells'
    chain runs on the CUs the big cells' reduction leaves idle.  (Holding the small cells'
    utilities back until the big cells' solves are done measured slower: 5.43 vs 5.12 ms, the
    big back-transform then shares the chip with them, profiles/r04_quad_after_solve_ab.json.)  beta / obj rows are written in
    place from cached launch plans, and the non-SPD systems are re-solved on the device inside
    each group's ridge launch (pivoted banded LU; no host sync, counts in ``LAST_REPAIRS``).
    """
    cell_src, cell_n = np.asarray(cell_src), np.asarray(cell_n)
    cell_scale = np.asarray(cell_scale, dtype=np.float64)
    job_cell, job_month, job_n = (np.asarray(job_cell), np.asarray(job_month),
                                  np.asarray(job_n))
    if not nat.is_device(SD):
        beta = ridge_grid(SD, Sr, cell_src, cell_n, cell_scale, lvec)
        return beta, quadform_utilities(D, R, beta, job_cell, job_month, job_n)
    sw = switches()
    split = sw.two_streams and len(np.unique(cell_n)) >= 2
    reset_coop_sync()
    th = _HostClock()
    S, P, _ = SD.shape
    check_launch_bounds(S, P, D.shape[0], cell_src, cell_n, job_cell, job_month, job_n)
    L = int(lvec.numel())
    nc = len(cell_src)
    dev = SD.device
    plan = _utilities_plan(P, L, dev, cell_src, cell_n, cell_scale, job_cell, job_month, job_n,
                           split=split, sw=sw)
    th("plans")
    # every [L, P] block is written whole by the ridge grid (zero padding past n included), so
    # no fill on the stream the big cells' chain forks from
    beta = torch.empty((nc, L, P), dtype=SD.dtype, device=dev)
    obj = torch.empty((len(job_cell), L), dtype=SD.dtype, device=dev)
    SD, Sr, D, R = SD.contiguous(), Sr.contiguous(), D.contiguous(), R.contiguous()
    lv = lvec.to(device=dev, dtype=torch.float64).contiguous()
    cur = torch.cuda.current_stream(dev)
    dv = plan["dv"]
    ng = len(plan["groups"])
    # big cells' factorisations issued first, on side streams; the small cells on `cur`
    streams = [_side_stream(dev, k) for k in range(ng - 1)] + [cur]
    for st in streams[:-1]:
        st.wait_stream(cur)
    counts = []
    for gi in range(ng):
        stream = streams[gi]
        _, _, rp, qp = plan["groups"][gi]
        with torch.cuda.stream(stream):
            cnt = ridge_launch(rp, dv[4 * gi], SD, Sr, lv, beta, d_wgmap=dv[4 * gi + 3], sw=sw)
            counts.append(cnt if cnt is not None else repair_launch(rp, dv[4 * gi], SD, Sr, lv, beta))
            quad_launch(qp, dv[4 * gi + 1], dv[4 * gi + 2], D, R, beta, obj, sw=sw)
    th("launch")
    for st in streams:
        if st == cur:
            continue
        cur.wait_stream(st)
        for t in (SD, Sr, D, R, lv, beta, obj, *counts):
            t.record_stream(st)
    LAST_REPAIRS[:] = counts
    return beta, obj


def quad_plan(P: int, L: int, Pb: int, job_cell, job_month, job_n, job_out=None,
              sw: Switches | None = None, run_steps: int | None = None,
              run_months: int | None = None, slots: int | None = None) -> dict:
    """Host-side descriptors of one utilities launch: JOB_DTYPE per job and ``tile_job``, one
    int32 ``job << 5 | row tile`` per 64-row tile in launch order.  ``job_out``: row of each
    job in the obj array the launch writes (default: 0..nj-1).

    ``run_steps`` / ``run_months`` (neither: one tile per workgroup, ``run_off`` None) select
    the run form: the months of every (cell, row tile) are cut into runs that one workgroup
    walks back to back (csrc/quadform.hip quad_pipe_body), and ``run_off`` holds the runs'
    offsets into ``tile_job``.  ``run_steps``: as many months per run as keep a run of the
    launch's longest tile within that many K steps and within the launch's K steps per
    workgroup slot (``slots``, default 3 per CU of a 256-CU chip: small launches keep fine
    work units), the same number for every tile of the launch and the months spread evenly
    over a group's runs - so a run is as much shorter as its tile is, and the launch, longest
    first, still ends on short work units (runs levelled to one length in K steps left the
    chip's tail idle and measured slower, profiles/r16_experiments.md).  ``run_months``:
    exactly that many months per run (the last run of a group takes what is left), whatever
    the launch's size.  Tiles that are not aligned stay runs of one.  Results do not depend
    on the runs (bitwise)."""
    sw = sw or switches()
    lib = nat.hip_lib()
    if lib.pfml_quadform_job_desc_size() != JOB_DTYPE.itemsize:
        raise RuntimeError("JobDesc layout mismatch between python and libpfml_hip")
    job_n = np.asarray(job_n)
    nj = len(job_n)
    # row tiles per job as the kernel counts them (the tail index n - 1 split off when n - 1
    # is a multiple of the K step: csrc/quadform.hip quad_main)
    tiles_of = {int(v): int(lib.pfml_quadform_row_tiles(int(v))) for v in np.unique(job_n)}
    ntile = np.array([tiles_of[int(v)] for v in job_n], dtype=np.int64)
    pt0 = np.concatenate([[0], np.cumsum(ntile)[:-1]]).astype(np.int32)
    desc = np.zeros(nj, dtype=JOB_DTYPE)
    desc["d_off"] = np.asarray(job_month, np.int64) * P * P
    desc["r_off"] = np.asarray(job_month, np.int64) * P
    desc["b_off"] = np.asarray(job_cell, np.int64) * L * Pb
    desc["o_off"] = (np.arange(nj, dtype=np.int64) if job_out is None
                     else np.asarray(job_out, np.int64)) * L
    desc["n"] = job_n.astype(np.int32)
    desc["ptile0"] = pt0
    if nj and int(ntile.max()) > 32:
        raise ValueError("quad_plan: more than 32 row tiles per job (n > 32 * 64)")
    jc = np.asarray(job_cell, np.int64)
    # jobs by (cell, n), stable: the validation months of a cell follow each other
    by_cell = np.lexsort((np.arange(nj), job_n, jc))
    jnt = ntile[by_cell]
    # tiles longest-first (row tile 0 of every job, then row tile 1, ...): the triangular K
    # loop of row tile rt is ~(n - 64 rt) long, so the launch ends on the short tiles;
    # entry = job << 5 | rt (the kernel writes partial slot ptile0 + rt of the job)
    jt = np.repeat(by_cell, jnt)
    rt = np.arange(len(jt), dtype=np.int64) - np.repeat(np.cumsum(jnt) - jnt, jnt)
    is_aligned = {n: bool(lib.pfml_quadform_aligned(n, L, P, Pb)) for n in tiles_of}
    run_off = None
    if len(jt) and (run_steps or run_months):
        jt, rt, run_off = _quad_runs(jt, rt, jc, job_n, is_aligned, run_steps,
                                     run_months, slots or QUAD_SLOTS_PER_CU * 256,
                                     sw.quad_xcd)
    else:
        order = np.argsort(rt, kind="stable")
        jt, rt = jt[order], rt[order]
        if len(jt) and sw.quad_xcd:
            order = _xcd_order(jc[jt])
            jt, rt = jt[order], rt[order]
    tile_job = ((jt << 5) | rt).astype(np.int32)
    return {"desc": desc, "tile_job": tile_job, "run_off": run_off, "nj": nj,
            "ntiles": len(jt), "nslots": int(ntile.sum()),
            "pipe": QUAD_PIPE if all(is_aligned.values()) else QUAD_PIPE_REST}


def quad_tile_steps(job_n, jt: np.ndarray, rt: np.ndarray) -> np.ndarray:
    """K steps of 16 of each tile (job jt, row tile rt): a row tile walks the indices from its
    own first row to the job's last (csrc/quadform.hip quad_main: a tail index n - 1 that is
    a multiple of 16 is not walked)."""
    n = np.asarray(job_n, np.int64)[jt]
    nmain = np.where((n > 1) & ((n - 1) % 16 == 0), n - 1, n)
    return -(-(nmain - 64 * rt) // 16)


def _quad_runs(jt, rt, jc, job_n, is_aligned, run_steps, run_months, slots, xcd):
    """Cut the tiles (jt, rt: cell-major, a cell's months in order, row tiles innermost) into
    runs - one (cell, n, row tile) over consecutive months of that group - order the runs
    longest first (per XCD queue when ``xcd``), and return the tiles in launch order with the
    runs' offsets."""
    steps = quad_tile_steps(job_n, jt, rt)
    cap = int(steps.sum()) // max(1, slots)        # the launch's K steps per workgroup slot
    # tiles by (cell, n, row tile), months in their order within
    order = np.lexsort((np.arange(len(jt)), rt, np.asarray(job_n)[jt], jc[jt]))
    jt, rt, steps = jt[order], rt[order], steps[order]
    key = np.stack([jc[jt], np.asarray(job_n, np.int64)[jt], rt], axis=1)
    new = np.concatenate([[True], (key[1:] != key[:-1]).any(axis=1)])
    starts = np.nonzero(new)[0]
    ends = np.concatenate([starts[1:], [len(jt)]])
    # months per run by the step target: what keeps a run of the launch's longest tile within
    # it and within the launch's steps per slot; every shorter tile gets as many months
    alig = np.array([is_aligned[int(v)] for v in np.asarray(job_n)[jt]])
    kmonths = max(1, min(int(run_steps or 0), cap) // int(steps[alig].max())) if alig.any() else 1
    offs = []                                      # run boundaries within the sorted tiles
    for a, b in zip(starts, ends):
        nm, st = int(b - a), int(steps[a])
        if not is_aligned[int(job_n[jt[a]])]:
            k = 1
        elif run_months:
            k = int(run_months)
        else:
            k = kmonths
        if run_months or k >= nm or k == 1:
            cuts = np.arange(a, b, max(1, min(k, nm)))
        else:                                      # level the group's runs
            nr = -(-nm // k)
            cuts = a + (np.arange(nr) * nm) // nr
        offs.append(cuts)
    r0 = np.concatenate(offs)
    r1 = np.concatenate([r0[1:], [len(jt)]])
    rlen = steps[r0] * (r1 - r0)
    rorder = np.argsort(-rlen, kind="stable")       # longest first
    if xcd:
        rorder = rorder[_xcd_order(jc[jt[r0[rorder]]])]
    r0, r1 = r0[rorder], r1[rorder]
    tiles = np.concatenate([np.arange(a, b) for a, b in zip(r0, r1)])
    run_off = np.concatenate([[0], np.cumsum(r1 - r0)]).astype(np.int32)
    return jt[tiles], rt[tiles], run_off


def quad_tables(plan: dict) -> np.ndarray:
    """The int32 table a utilities launch reads on the device: ``tile_job``, followed by the
    runs' offsets when the plan has runs (``quad_launch`` tells them apart by the plan)."""
    if plan["run_off"] is None:
        return plan["tile_job"]
    return np.concatenate([plan["tile_job"], plan["run_off"]]).astype(np.int32)


NXCD = 8   # MI355X: workgroup b of a launch is dispatched to XCD b mod 8


def _xcd_order(cell: np.ndarray) -> np.ndarray:
    """Launch order of a utilities launch's work units (tiles, or runs of tiles; given in
    their longest-first order, which is kept per XCD) so that every unit of one cell runs on
    XCD ``cell mod 8``: slot s of the launch goes to XCD s mod 8 and takes the next unit of
    that XCD's queue (cells numbered densely within the launch).  A cell's beta block (L x n,
    ~0.4 MB at n = 513) is then read by its 12 months x row tiles through ONE L2 instead of
    all eight - in launch order every XCD saw every cell, and the L2s kept re-fetching beta
    from HBM.  Queues that run dry hand their slots to the longest remaining one (the tail
    loses the affinity, not the order)."""
    _, x = np.unique(np.asarray(cell, np.int64), return_inverse=True)   # dense cell ranks
    x = x.reshape(-1) % NXCD
    queues = [list(np.nonzero(x == k)[0]) for k in range(NXCD)]
    heads = [0] * NXCD
    order = np.empty(len(x), dtype=np.int64)
    for s in range(len(x)):
        k = s % NXCD
        if heads[k] >= len(queues[k]):
            k = int(np.argmax([len(q) - h for q, h in zip(queues, heads)]))
        order[s] = queues[k][heads[k]]
        heads[k] += 1
    return order


def quad_launch(plan: dict, d_desc: torch.Tensor, d_tj: torch.Tensor, D: torch.Tensor,
                R: torch.Tensor, beta: torch.Tensor, obj: torch.Tensor,
                sw: Switches | None = None) -> None:
    """Queue one utilities launch (csrc/quadform.hip) of a ``quad_plan`` made for these P, L
    and beta row stride; ``d_tj`` is the device copy of ``quad_tables(plan)``.  Default: the
    pipelined loop for the aligned jobs - QUAD_PIPE when every job is aligned, as in
    production, else QUAD_PIPE_REST, which adds a launch of the direct form's loop for the
    rest - over the plan's runs when it has any.  ``sw.quad_direct``: the direct form for
    every tile, one per workgroup (the runs are not used)."""
    sw = sw or switches()
    if plan["nj"] == 0:
        return
    P = D.shape[-1]
    L, Pb = beta.shape[1], beta.shape[2]
    partial = torch.empty((plan["nslots"], L), dtype=torch.float64, device=D.device)
    lib = nat.hip_lib()
    args = (D.data_ptr(), P, R.data_ptr(), beta.data_ptr(), Pb, d_desc.data_ptr(), plan["nj"],
            d_tj.data_ptr(), plan["ntiles"])
    tail = (L, partial.data_ptr(), obj.data_ptr(), nat.stream_of(D))
    run_off = plan.get("run_off")
    if run_off is None or sw.quad_direct:
        form = QUAD_DIRECT if sw.quad_direct else plan["pipe"]
        nat.check(lib.pfml_quadform(*args, form, *tail), "pfml_quadform")
        return
    if d_tj.numel() * d_tj.element_size() != 4 * (plan["ntiles"] + len(run_off)):
        raise ValueError("quad_launch: the plan has runs, so d_tj must be the upload of "
                         "quad_tables(plan) (tile_job followed by run_off)")
    nat.check(lib.pfml_quadform_runs(*args, d_tj.data_ptr() + 4 * plan["ntiles"],
                                     len(run_off) - 1, plan["pipe"], *tail),
              "pfml_quadform")       # one name for the utilities launch, whichever entry


def quadform_utilities(D: torch.Tensor, R: torch.Tensor, beta: torch.Tensor,
                       job_cell: np.ndarray, job_month: np.ndarray, job_n: np.ndarray
                       ) -> torch.Tensor:
    """obj[j, l] = R[m_j,:n]·beta[c_j,l,:n] - 1/2 beta[c_j,l,:n]' D[m_j,:n,:n] beta[c_j,l,:n]."""
    T, P, _ = D.shape
    nc, L, Pb = beta.shape
    nj = len(job_cell)
    obj = torch.empty((nj, L), dtype=D.dtype, device=D.device)
    if nj == 0:
        return obj
    if nat.is_device(D):
        sw = switches()
        plan = quad_plan(P, L, Pb, job_cell, job_month, job_n, sw=sw, run_steps=QUAD_RUN_STEPS,
                         slots=QUAD_SLOTS_PER_CU * num_cus(D.device))
        d_desc, d_tj = upload([plan["desc"], quad_tables(plan)], D.device)
        quad_launch(plan, d_desc, d_tj, D.contiguous(), R.contiguous(), beta.contiguous(), obj, sw)
        return obj
    for j in range(nj):
        n, m, c = int(job_n[j]), int(job_month[j]), int(job_cell[j])
        Bm = beta[c, :, :n]                       # [L, n]
        quad = ((Bm @ D[m, :n, :n]) * Bm).sum(1)
        obj[j] = Bm @ R[m, :n] - 0.5 * quad
    return obj
