"""The case table of the tiled MFMA GEMM's tests (launch_gemm_tiled / k_gemm_tiled, csrc/kernels_gemm.hip) and the list of
launch forms it has to reach.  Plain data plus the plan query (include/ftcf.h ftcf_gemm_tiled_plan, host only): imported by
test_gemm_tiled_plan_host.py, which asks the query for every case and fails when a form is no longer reached, and by
test_gpu_tiled_gemm.py, which runs the cases.

A case is (int8, m, n, k, splitk): splitk None = the launcher's default, "0" = FTCF_GEMM_SPLITK=0 (no split-K: the 32-row form
up to 32 rows and the one-workgroup-per-tile forms above).  The cases are grouped by weight matrix (int8, k, n), so that a test
generates and tiles a matrix once.  The row counts typed in below are starting points taken from the launcher's constants; the
query is the judge: when a threshold moves, the host test names the form or the row step that the table no longer covers."""
import contextlib
import ctypes as C
import os
from collections import namedtuple

Case = namedtuple("Case", "int8 m n k splitk")
Group = namedtuple("Group", "int8 k n cases")

SPLITK, ROWS32, ONE_WG, FOUR_WAVE = 0, 1, 2, 3  # ftcf_gemm_plan.family
FAMILY_NAMES = {SPLITK: "split-K", ROWS32: "32-row form", ONE_WG: "one workgroup per tile", FOUR_WAVE: "four-wave form"}

# rows above which split-K tiles are 128 rows high, and the last split-K row count (kernels_gemm.hip GEMM_SK128_MIN_M_*,
# GEMM_SPLITK_MAX_M_*)
_SK128 = {True: 320, False: 192}
_LAST = {True: 384, False: 768}


def _split_rows(int8):
    """both sides of every row step of the split-K family, and one row count in the middle of the 64-row range"""
    return (17, 32, 33, 48, 49, 64, 65, 129, _SK128[int8], _SK128[int8] + 1, _LAST[int8], _LAST[int8] + 1)


def _groups(int8):
    last, first_big = _LAST[int8], _LAST[int8] + 1
    t = []

    def add(k, n, rows, unsplit_rows=()):
        t.append(Group(int8, k, n, tuple([Case(int8, m, n, k, None) for m in rows] + [Case(int8, m, n, k, "0") for m in unsplit_rows])))

    # split-K.  k-steps of 64: 80 = ring, 7 slices of 12 (the last one 8); 65 = plain, 8 slices of 9 (the last one 2); 16 = ring, two
    # slices; 17 = plain, 9 + 8; 4 = ring, one slice; 9 = plain, one slice; 1 = a single k-step.  n: 16 = one column tile; 272 = one
    # 256-column block plus one tile; 1280 = 5 blocks (the grid rounds them to 8: idle workgroups); 5120 = 20 blocks
    add(5120, 272, _split_rows(int8), unsplit_rows=(17, 32, 33, 48, 49, 64, 200))
    add(4160, 1280, _split_rows(int8), unsplit_rows=(17, 33, 64, 200))
    add(1024, 16, (17, 33, 65, 129, last), unsplit_rows=(17, 48))
    add(1088, 5120, (17, 64, 65, last))
    add(256, 272, (17, 48, 200))
    add(576, 1280, (32, 49, last))
    add(64, 16, (17, 65))
    # one workgroup per tile, the first row count past split-K: 2 k-steps = ring of two, 3 = plain loop.  The tile height and
    # `lone` (at most 256 tiles) follow n: see FORMS.  1024 / 1025 rows at n = 5120: 160 128-row tiles against 180, which above
    # 1024 rows makes 64-row tiles.  2048 / 2049 rows at n = 4096: the four-wave form (fp16 weights), 16 and 17 row blocks
    for k in (128, 192):
        add(k, 16, (first_big,))
        add(k, 272, (first_big,))
        add(k, 5120, (first_big, 1024, 1025))
        add(k, 8192, (first_big,))
        add(k, 9472, (first_big,))
        add(k, 10240, (first_big,))
        add(k, 16640, (first_big,))
        add(k, 4096, (2048, 2049))
    return t


GROUPS = _groups(True) + _groups(False)
CASES = [c for g in GROUPS for c in g.cases]


def group_id(g):
    return f"{'int8' if g.int8 else 'fp16'}-k{g.k}-n{g.n}"


def case_id(c):
    return f"{'int8' if c.int8 else 'fp16'}-m{c.m}-n{c.n}-k{c.k}" + ("" if c.splitk is None else f"-splitk{c.splitk}")


@contextlib.contextmanager
def splitk_env(value):
    """FTCF_GEMM_SPLITK as the launcher and the query read it at every call (None: unset)"""
    old = os.environ.get("FTCF_GEMM_SPLITK")
    try:
        if value is None:
            os.environ.pop("FTCF_GEMM_SPLITK", None)
        else:
            os.environ["FTCF_GEMM_SPLITK"] = value
        yield
    finally:
        if old is None:
            os.environ.pop("FTCF_GEMM_SPLITK", None)
        else:
            os.environ["FTCF_GEMM_SPLITK"] = old


def query(capi, int8, m, n, k, has_workspace):
    p = capi.GemmPlan()
    capi.check(capi.lib().ftcf_gemm_tiled_plan(m, n, k, int(int8), int(has_workspace), C.byref(p)))
    return p


_entry_max_m = {}


def entry_workspace_max_m(capi):
    """the row count up to which ftcf_fpA_intB_gemm / ftcf_fp16_gemm hold a split-K workspace (capi_kernels.hip
    abi_gemm_workspace: 17 <= m <= gemm_tiled_splitk_max_m(), the larger of the two weight types' limits), found by asking"""
    key = os.environ.get("FTCF_GEMM_SPLITK_MAX_M")
    if key not in _entry_max_m:
        with splitk_env(None):
            _entry_max_m[key] = max([16] + [m for int8 in (True, False) for m in range(17, 4097)
                                            if query(capi, int8, m, 272, 256, True).family == SPLITK])
    return _entry_max_m[key]


def plan(capi, c):
    """the form the public GEMM entry points run case c in"""
    has_ws = 17 <= c.m <= entry_workspace_max_m(capi)
    with splitk_env(c.splitk):
        return query(capi, c.int8, c.m, c.n, c.k, has_ws)


def describe(p):
    return (f"{FAMILY_NAMES[p.family]}, {p.tile_rows}-row tiles, gx {p.gx} gy {p.gy}, {p.slices} slice(s) of {p.steps_per_slice} k-steps, "
            f"ring {p.ring}, prefetch {p.prefetch}, two per CU {p.two_per_cu}, lone {p.lone}, grid {p.grid}")


def _ragged(c, p):
    return p.slices > 1 and (c.k // 64) % p.steps_per_slice != 0


def _sk(pred):
    return lambda c, p: c.splitk is None and p.family == SPLITK and pred(c, p)


def _wg(pred):
    return lambda c, p: c.splitk is None and p.family == ONE_WG and pred(c, p)


# (name, weight types, predicate(case, plan)): every launch form the table has to reach, for each of the named weight types
BOTH, FP16_ONLY = (True, False), (False,)
FORMS = [
    ("split-K, 32-row tile", BOTH, _sk(lambda c, p: p.tile_rows == 32 and p.gy == 1)),
    ("split-K, 48-row tile", BOTH, _sk(lambda c, p: p.tile_rows == 48 and p.gy == 1)),
    ("split-K, 64-row tile, one row block", BOTH, _sk(lambda c, p: p.tile_rows == 64 and p.gy == 1)),
    ("split-K, 64-row tiles, several row blocks", BOTH, _sk(lambda c, p: p.tile_rows == 64 and p.gy > 1)),
    ("split-K, 128-row tiles", BOTH, _sk(lambda c, p: p.tile_rows == 128 and p.gy > 1)),
    ("split-K, ring of four, 1 slice", BOTH, _sk(lambda c, p: p.ring == 4 and p.prefetch == 1 and p.slices == 1)),
    ("split-K, plain loop, 1 slice", BOTH, _sk(lambda c, p: p.ring == 0 and p.prefetch == 0 and p.slices == 1)),
    ("split-K, a single k-step", BOTH, _sk(lambda c, p: c.k == 64)),
    ("split-K, ring of four, 2 slices", BOTH, _sk(lambda c, p: p.ring == 4 and p.slices == 2)),
    ("split-K, plain loop, 2 slices", BOTH, _sk(lambda c, p: p.ring == 0 and p.slices == 2)),
    ("split-K, ring of four, 7 or 8 slices", BOTH, _sk(lambda c, p: p.ring == 4 and p.slices in (7, 8))),
    ("split-K, plain loop, 7 or 8 slices", BOTH, _sk(lambda c, p: p.ring == 0 and p.slices in (7, 8))),
    ("split-K, ring of four, ragged last slice", BOTH, _sk(lambda c, p: p.ring == 4 and _ragged(c, p))),
    ("split-K, plain loop, ragged last slice", BOTH, _sk(lambda c, p: p.ring == 0 and _ragged(c, p))),
    ("split-K, 128-row tiles, ragged last slice", BOTH, _sk(lambda c, p: p.tile_rows == 128 and _ragged(c, p))),
    ("split-K, n = 16", BOTH, _sk(lambda c, p: c.n == 16)),
    ("split-K, n = whole 256-column blocks plus one tile", BOTH, _sk(lambda c, p: c.n > 256 and c.n % 256 == 16)),
    ("split-K, idle workgroups (column blocks not a multiple of 8)", BOTH, _sk(lambda c, p: p.gx % 8 != 0 and p.gx > 1)),
    ("one workgroup per tile, 64-row, ring of two, lone", BOTH, _wg(lambda c, p: p.tile_rows == 64 and p.ring == 2 and p.lone == 1)),
    ("one workgroup per tile, 64-row, ring of two, not lone", BOTH, _wg(lambda c, p: p.tile_rows == 64 and p.ring == 2 and p.lone == 0)),
    ("one workgroup per tile, 64-row, plain loop", BOTH, _wg(lambda c, p: p.tile_rows == 64 and p.ring == 0)),
    ("one workgroup per tile, 128-row, ring of two, lone", BOTH, _wg(lambda c, p: p.tile_rows == 128 and p.ring == 2 and p.lone == 1)),
    ("one workgroup per tile, 128-row, ring of two, not lone", BOTH, _wg(lambda c, p: p.tile_rows == 128 and p.ring == 2 and p.lone == 0)),
    ("one workgroup per tile, 128-row, plain loop", BOTH, _wg(lambda c, p: p.tile_rows == 128 and p.ring == 0)),
    ("one workgroup per tile, prefetch", BOTH, _wg(lambda c, p: p.prefetch == 1 and p.two_per_cu == 0)),
    ("one workgroup per tile, two per CU", (True,), _wg(lambda c, p: p.prefetch == 0 and p.two_per_cu == 1)),
    ("one workgroup per tile, 64-row tiles above 1024 rows where 128-row tiles would be 160..255",
     BOTH, _wg(lambda c, p: p.tile_rows == 64 and c.m > 1024 and 160 <= p.gx * ((c.m + 127) // 128) < 256)),
    ("one workgroup per tile, 128-row tiles at 1024 rows", BOTH, _wg(lambda c, p: p.tile_rows == 128 and c.m == 1024)),
    ("one workgroup per tile, n = 16", BOTH, _wg(lambda c, p: c.n == 16)),
    ("one workgroup per tile, n = whole 256-column blocks plus one tile", BOTH, _wg(lambda c, p: c.n > 256 and c.n % 256 == 16)),
    ("one workgroup per tile, idle workgroups", BOTH, _wg(lambda c, p: p.gx % 8 != 0 and p.gx > 1)),
    ("one workgroup per tile, ragged last row block", BOTH, _wg(lambda c, p: c.m % p.tile_rows != 0 and p.gy > 1)),
    ("four-wave form, whole row blocks", FP16_ONLY, lambda c, p: p.family == FOUR_WAVE and c.m % 128 == 0),
    ("four-wave form, ragged last row block", FP16_ONLY, lambda c, p: p.family == FOUR_WAVE and c.m % 128 != 0),
    ("four-wave form, plain loop on an even and an odd k-step count (even)", FP16_ONLY,
     lambda c, p: p.family == FOUR_WAVE and (c.k // 64) % 2 == 0),
    ("four-wave form, plain loop on an even and an odd k-step count (odd)", FP16_ONLY,
     lambda c, p: p.family == FOUR_WAVE and (c.k // 64) % 2 == 1),
    ("FTCF_GEMM_SPLITK=0, 32-row form", BOTH, lambda c, p: c.splitk == "0" and p.family == ROWS32 and c.m > 16),
    ("FTCF_GEMM_SPLITK=0, 32-row form, 32 rows", BOTH, lambda c, p: c.splitk == "0" and p.family == ROWS32 and c.m == 32),
    ("FTCF_GEMM_SPLITK=0, 32-row form, n = 16", BOTH, lambda c, p: c.splitk == "0" and p.family == ROWS32 and c.n == 16),
    ("FTCF_GEMM_SPLITK=0, one workgroup per tile at 33..64 rows, ring of two",
     BOTH, lambda c, p: c.splitk == "0" and p.family == ONE_WG and 33 <= c.m <= 64 and p.ring == 2),
    ("FTCF_GEMM_SPLITK=0, one workgroup per tile at 33..64 rows, plain loop",
     BOTH, lambda c, p: c.splitk == "0" and p.family == ONE_WG and 33 <= c.m <= 64 and p.ring == 0),
    ("FTCF_GEMM_SPLITK=0, one workgroup per tile at 200 rows", BOTH, lambda c, p: c.splitk == "0" and p.family == ONE_WG and c.m == 200),
]


def reached(capi):
    """{(form name, int8): [cases that reach it, in table order]}"""
    out = {(name, int8): [] for name, types, _ in FORMS for int8 in types}
    for c in CASES:
        p = plan(capi, c)
        for name, types, pred in FORMS:
            if c.int8 in types and pred(c, p):
                out[(name, c.int8)].append(c)
    return out


def one_case_per_form(capi):
    """the first case of the table that reaches each form, without repeats, in table order: what the Gaussian test and the
    bias + gelu test run"""
    picked = {cs[0] for cs in reached(capi).values() if cs}
    return [c for c in CASES if c in picked]
