"""The FFT routes no other test reaches (CPU: the host SIMT emulator, and the host-only route query on the gfx950 product library as well).

``fft_route()`` (lama_amd/csrc/fft.hip) picks one of six kernel families from the plane size, the element type and the ALIGNMENT of the
views and of the workspace.  Every other FFT test builds its views with ``L.view()`` on fresh tensors -- 16-byte aligned, dense batch
stride -- so the alignment fallbacks of family 1, the separable DFT (family 6) and the fp16 instances of families 5 and 6 ran in no test.
Here every case first asserts its route through ``lama_fft_route_query`` (a test can only claim a route it can see), then transforms both
ways -- the inverse with and without a residual -- against float64 numpy.fft at the bars of tests/fft_route_util.py, inside hand-placed,
sentinel-guarded views.  ``-s`` prints one line per check.  tests/test_fft_routes_gpu.py runs the same checks on the MI355X.

The pinned routes are read off ``fft_route()`` and the table at the top of fft.hip, not copied from the query.  One of them differs from
the list the tests were specified with: a 256 x 32 plane is 4352 float2 of LDS and fits ONE 256-thread workgroup of the one-launch
mixed-radix kernel (row 2 of the table comes before row 4, and ``mr_threads`` takes it), so it is family 2, not the two-pass family 4;
the comment table and the code agree on that.  Family 4 on a NON-square plane is therefore pinned and run at 512 x 128, the smallest
power-of-two rectangle that one workgroup cannot hold (512 * 65 float2 > 20480).

Host-only checks (fake, never dereferenced addresses) run on BOTH libraries: the emulator is the profiling build, the product routing table
is only tested through the product library, which loads without a GPU (tests/test_abi.py relies on the same).

  * the route table;
  * direction symmetry: rfft2 and irfft2 return the same code and family for every plane of h in {2, 135} x w in 2 .. 2048 and w in {2, 240} x
    h in 2 .. 2048, both dtypes.  Before the fix of the separable DFT's LDS bound (it was sized per direction, and the inverse rows need
    more) this failed on 284 widths between 1196 and 1599 at h = 2: served forward, refused inverse;
  * the advertised workspace is enough: no LAMA_ERR_WORKSPACE with ``lama_fft_workspace_bytes``, and none needed where that is 0."""
import functools

import pytest
import torch

from lama_amd import _lib as L
from tests import fft_route_util as U
from tests.emu import emu_lib

F32, F16 = torch.float32, torch.float16
IP64, IP128, SIZED, GENERIC = L.FFT_KIND_IP64, L.FFT_KIND_IP128, L.FFT_KIND_SIZED, L.FFT_KIND_GENERIC
REAL_A, SPEC_A, WS_A = 0x10000000, 0x20000000, 0x40000000          # fake 16-byte aligned addresses of the host-only checks


def test_published_kinds_match_the_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lama_hip.h')).read()
    kinds = {k: int(v) for k, v in re.findall(r'#define LAMA_FFT_KIND_([A-Z0-9]+) (\d+)', src)}
    assert kinds == dict(WINO64=L.FFT_KIND_WINO64, IP64=IP64, IP128=IP128, TRACE64=L.FFT_KIND_TRACE64, SEQ=L.FFT_KIND_SEQ, SIZED=SIZED, GENERIC=GENERIC)


# ---- host-only: the route query on fake addresses ----------------------------------------------------------------------------------------

@functools.lru_cache(None)
def product_lib():
    from lama_amd import build as B
    return L.LamaLib(B.build(verbose=False))          # the gfx950 library: loads without a GPU, its pure host functions work


@pytest.fixture(params=['emulator', 'product'])
def hostlib(request):
    return emu_lib() if request.param == 'emulator' else product_lib()


def fake_query(lib, h, w, B, C, dtype, inverse, variant='aligned', ws='advertised', resid=True, masked=False):
    """The query for views at fake addresses: ``variant`` as in U.VARIANTS; ``ws``: 'advertised' (lama_fft_workspace_bytes at an aligned
    address; none where that is 0), 'none', or a byte shift of the advertised one."""
    v = U.VARIANTS[variant]
    es = 2 if dtype == F16 else 4
    dt = L.DT_F16 if dtype == F16 else L.DT_F32
    wf = w // 2 + 1
    real = L.Tensor4(REAL_A + es * v['real_off'], C * h * w + v['pad'], C, h, w, dt)
    res = L.Tensor4(REAL_A + 0x8000000 + es * v['real_off'], C * h * w + v['pad'], C, h, w, dt)
    spec = L.Tensor4(SPEC_A + es * v['spec_off'], 2 * C * h * wf + v['pad'], 2 * C, h, wf, dt)
    mask = None
    if masked:          # laid out like the output, always fp32
        mask = L.Tensor4(0x30000000, C * h * w, C, h, w, L.DT_F32) if inverse else L.Tensor4(0x30000000, 2 * C * h * wf, 2 * C, h, wf, L.DT_F32)
    need = lib.fft_workspace_bytes(B, C, h, w)
    addr, nbytes = (WS_A + 4 * v['ws_shift'], need) if need else (None, 0)
    if ws == 'none':
        addr, nbytes = None, 0
    return lib.fft_route_query(real, res if (inverse and resid) else None, spec, B, inverse, addr, nbytes, mask=mask)


# (h, w, B, C, dtype, variant, workspace, expected): expected = (family, kind) or a LAMA_ERR_* code; read off fft_route() (module docstring)
ROUTE_TABLE = [
    (64, 64, 2, 3, F32, 'aligned', 'advertised', (1, IP64)),
    (64, 64, 2, 3, F32, 'spec+1', 'advertised', (1, SIZED)),
    (64, 64, 2, 3, F32, 'real+1', 'advertised', (2, 256)),
    (64, 64, 2, 3, F32, 'stride+2', 'advertised', (2, 256)),
    (128, 128, 2, 3, F32, 'aligned', 'advertised', (1, IP128)),
    (128, 128, 2, 3, F32, 'spec+1', 'advertised', (1, SIZED)),
    (128, 128, 2, 3, F32, 'real+1', 'advertised', (2, 1024)),
    (128, 128, 2, 3, F32, 'stride+2', 'advertised', (2, 1024)),
    (32, 32, 2, 4, F32, 'aligned', 'advertised', (1, SIZED)),            # 8 planes: whole workgroups of 4
    (32, 32, 2, 3, F32, 'aligned', 'advertised', (1, GENERIC)),          # 6 planes: a ragged last workgroup
    (16, 32, 2, 3, F32, 'aligned', 'advertised', (1, GENERIC)),
    (256, 256, 1, 2, F32, 'aligned', 'advertised', (3, 0)),
    (256, 256, 1, 2, F32, 'aligned', 'none', L.ERR_WORKSPACE),
    (256, 256, 1, 2, F32, 'ws+4', 'advertised', (4, 0)),
    (256, 256, 1, 2, F32, 'real+1', 'advertised', (4, 0)),
    (256, 256, 1, 2, F16, 'aligned', 'advertised', (4, 0)),
    (256, 32, 2, 3, F32, 'aligned', 'advertised', (2, 256)),             # NOT family 4: module docstring
    (512, 128, 1, 2, F32, 'aligned', 'advertised', (4, 0)),
    (512, 128, 1, 2, F16, 'aligned', 'advertised', (4, 0)),
    (45, 60, 2, 3, F32, 'aligned', 'advertised', (2, 256)),
    (90, 160, 2, 3, F32, 'aligned', 'advertised', (2, 1024)),
    (270, 480, 2, 3, F32, 'aligned', 'advertised', (5, 0)),
    (2, 1028, 1, 2, F32, 'aligned', 'advertised', (6, 0)),               # 1028 = 4 * 257: the radix-4 pass needs 257 > 256 threads per transform
    (4, 1028, 1, 2, F32, 'aligned', 'advertised', (6, 0)),
    (16, 1028, 1, 2, F32, 'aligned', 'advertised', (2, 1024)),           # ... which the 1024-thread workgroup of a plane this large has
    (2, 1204, 1, 2, F32, 'aligned', 'advertised', L.ERR_UNSUPPORTED),    # the DFT's inverse rows need 165536 bytes of LDS: refused both ways
    (2, 1286, 1, 2, F32, 'aligned', 'advertised', L.ERR_UNSUPPORTED),
]
# the masked entries: served by family 3 only
MASKED_TABLE = [
    (256, 256, 1, 2, F32, 'aligned', 'advertised', (3, 0)),
    (256, 256, 1, 2, F32, 'aligned', 'none', L.ERR_WORKSPACE),
    (256, 256, 1, 2, F32, 'real+1', 'advertised', L.ERR_UNSUPPORTED),
    (256, 256, 1, 2, F32, 'ws+4', 'advertised', L.ERR_UNSUPPORTED),
    (256, 256, 1, 2, F16, 'aligned', 'advertised', L.ERR_UNSUPPORTED),
    (64, 64, 2, 3, F32, 'aligned', 'advertised', L.ERR_UNSUPPORTED),
    (128, 128, 2, 3, F32, 'aligned', 'advertised', L.ERR_UNSUPPORTED),
    (256, 32, 2, 3, F32, 'aligned', 'advertised', L.ERR_UNSUPPORTED),
    (45, 60, 2, 3, F32, 'aligned', 'advertised', L.ERR_UNSUPPORTED),
    (270, 480, 2, 3, F32, 'aligned', 'advertised', L.ERR_UNSUPPORTED),
]


def _row_id(r):
    return f'{r[0]}x{r[1]}-B{r[2]}C{r[3]}-{U.DT_NAME[r[4]]}-{r[5]}' + ('' if r[6] == 'advertised' else '-ws_' + r[6])


def _expect(want):
    return (want, None, None) if isinstance(want, int) else (0,) + tuple(want)


@pytest.mark.parametrize('row', ROUTE_TABLE, ids=_row_id)
def test_route_table(hostlib, row):
    h, w, B, C, dtype, variant, ws, want = row
    for inverse, resid in ((False, False), (True, True), (True, False)):
        got = fake_query(hostlib, h, w, B, C, dtype, inverse, variant, ws, resid)
        assert got == _expect(want), (row[:7], inverse, resid, got)


@pytest.mark.parametrize('row', MASKED_TABLE, ids=_row_id)
def test_route_table_masked(hostlib, row):
    h, w, B, C, dtype, variant, ws, want = row
    for inverse in (False, True):
        got = fake_query(hostlib, h, w, B, C, dtype, inverse, variant, ws, masked=True)
        assert got == _expect(want), (row[:7], inverse, got)


def test_route_query_rejects_what_the_entries_reject(hostlib):
    ok = L.Tensor4(REAL_A, 2 * 64 * 64, 2, 64, 64, L.DT_F32)
    spec = L.Tensor4(SPEC_A, 4 * 64 * 33, 4, 64, 33, L.DT_F32)
    assert hostlib.fft_route_query(ok, None, spec, 1, False) == (0, 1, IP64)
    assert hostlib.fft_route_query(ok, None, L.Tensor4(SPEC_A, 4 * 64 * 32, 4, 64, 32, L.DT_F32), 1, False)[0] == L.ERR_BAD_ARG      # wrong spectrum width
    assert hostlib.fft_route_query(ok, None, L.Tensor4(SPEC_A, 4 * 64 * 33, 4, 64, 33, L.DT_F16), 1, False)[0] == L.ERR_UNSUPPORTED   # mixed dtypes
    assert hostlib.fft_route_query(ok, None, spec, 0, False)[0] == L.ERR_BAD_ARG
    assert hostlib.fft_route_query(L.Tensor4(None, 2 * 64 * 64, 2, 64, 64, L.DT_F32), None, spec, 1, True)[0] == L.ERR_BAD_ARG
    assert hostlib.fft_route_query(ok, L.Tensor4(REAL_A, 64 * 64, 1, 64, 64, L.DT_F32), spec, 1, True)[0] == L.ERR_BAD_ARG            # resid of another shape


def sweep_planes():
    for h in (2, 135):
        for w in range(2, 2049):
            yield h, w
    for w in (2, 240):
        for h in range(2, 2049):
            yield h, w


@pytest.mark.parametrize('dtype', [F32, F16], ids=['fp32', 'fp16'])
def test_direction_symmetry_and_workspace_sweep(hostlib, dtype):
    """Both directions return the same code and family for every plane of the sweep, and the advertised workspace is enough."""
    B, C = 1, 2
    asym, short, served = [], [], {}
    for h, w in sweep_planes():
        f = fake_query(hostlib, h, w, B, C, dtype, False)
        i = fake_query(hostlib, h, w, B, C, dtype, True)
        if f[:2] != i[:2] or fake_query(hostlib, h, w, B, C, dtype, True, resid=False)[:2] != f[:2]:
            asym.append((h, w, f, i))
        if L.ERR_WORKSPACE in (f[0], i[0]):
            short.append((h, w, f, i))
        if hostlib.fft_workspace_bytes(B, C, h, w) == 0 and (f[0] or i[0]):
            short.append((h, w, f, i))
        served[f[1]] = served.get(f[1], 0) + 1
    print(f'[fft-routes] sweep {U.DT_NAME[dtype]}: planes per family (None = refused in both directions) {dict(sorted(served.items(), key=str))}')
    assert not asym, f'{len(asym)} planes served in one direction only, first {asym[:3]}'
    assert not short, f'{len(short)} planes not served with the advertised workspace, first {short[:3]}'
    assert served.get(6, 0) > 0          # the sweep reaches the family whose bound it is about


# ---- numeric: the emulator -------------------------------------------------------------------------------------------------------------------

# (h, w, B, C, dtype, variant, (family, kind))
ALIGN_F32 = [
    (64, 64, 2, 3, F32, 'aligned', (1, IP64)), (64, 64, 2, 3, F32, 'real+1', (2, 256)), (64, 64, 2, 3, F32, 'spec+1', (1, SIZED)),
    (64, 64, 2, 3, F32, 'stride+2', (2, 256)),
    (128, 128, 2, 3, F32, 'aligned', (1, IP128)), (128, 128, 2, 3, F32, 'real+1', (2, 1024)), (128, 128, 2, 3, F32, 'spec+1', (1, SIZED)),
    (128, 128, 2, 3, F32, 'stride+2', (2, 1024)),
    (32, 32, 2, 4, F32, 'aligned', (1, SIZED)), (32, 32, 2, 4, F32, 'real+1', (2, 256)), (32, 32, 2, 4, F32, 'spec+1', (1, SIZED)),
    (32, 32, 2, 4, F32, 'stride+2', (2, 256)),
    (32, 32, 2, 3, F32, 'aligned', (1, GENERIC)), (32, 32, 2, 3, F32, 'real+1', (2, 256)), (32, 32, 2, 3, F32, 'spec+1', (1, GENERIC)),
    (32, 32, 2, 3, F32, 'stride+2', (2, 256)),
    (16, 32, 2, 3, F32, 'aligned', (1, GENERIC)), (16, 32, 2, 3, F32, 'real+1', (2, 256)), (16, 32, 2, 3, F32, 'spec+1', (1, GENERIC)),
    (16, 32, 2, 3, F32, 'stride+2', (2, 256)),
    (256, 32, 2, 3, F32, 'aligned', (2, 256)), (256, 32, 2, 3, F32, 'real+1', (2, 256)), (256, 32, 2, 3, F32, 'spec+1', (2, 256)),
    (256, 32, 2, 3, F32, 'stride+2', (2, 256)),
    (256, 256, 1, 2, F32, 'aligned', (3, 0)), (256, 256, 1, 2, F32, 'real+1', (4, 0)), (256, 256, 1, 2, F32, 'spec+1', (3, 0)),
    (256, 256, 1, 2, F32, 'stride+2', (4, 0)), (256, 256, 1, 2, F32, 'ws+4', (4, 0)),
    (512, 128, 1, 2, F32, 'aligned', (4, 0)), (512, 128, 1, 2, F32, 'real+1', (4, 0)),       # family 4 on a non-square plane (module docstring)
]
ALIGN_F16 = [
    (64, 64, 2, 3, F16, 'aligned', (1, IP64)), (64, 64, 2, 3, F16, 'real+1', (2, 256)), (64, 64, 2, 3, F16, 'real+2', (2, 256)),
    (64, 64, 2, 3, F16, 'spec+1', (1, GENERIC)),          # no sized fp16 instance of the two-buffer kernels at 64 / 128
    (128, 128, 2, 3, F16, 'aligned', (1, IP128)), (128, 128, 2, 3, F16, 'real+1', (2, 1024)), (128, 128, 2, 3, F16, 'real+2', (2, 1024)),
    (128, 128, 2, 3, F16, 'spec+1', (1, GENERIC)),
    (32, 32, 2, 4, F16, 'aligned', (1, SIZED)), (32, 32, 2, 4, F16, 'real+1', (2, 256)), (32, 32, 2, 4, F16, 'real+2', (2, 256)),
    (32, 32, 2, 4, F16, 'spec+1', (1, SIZED)),
    (512, 128, 1, 2, F16, 'aligned', (4, 0)), (512, 128, 1, 2, F16, 'real+2', (4, 0)),       # fp16 I/O of family 4 on a non-square plane
]
DFT_PRODUCTION = [(2, 1028, 1, 2, F32, 'aligned', (6, 0)), (4, 1028, 1, 2, F32, 'aligned', (6, 0))]
# LAMA_FFT_MR = 0 (profiling build): no mixed-radix kernels, every plane that is not a power of two in 16 .. 1024 takes the separable DFT
DFT_FORCED = [(h, w, 2, 3, F32, 'aligned', (6, 0)) for (h, w) in [(45, 60), (21, 94), (61, 67), (17, 16), (13, 13), (3, 2), (1, 16), (24, 40), (90, 160), (8, 12)]] + \
             [(h, w, 2, 3, F16, 'aligned', (6, 0)) for (h, w) in [(45, 60), (21, 94), (61, 67)]]
# LAMA_FFT_MR = 2: the two-launch mixed-radix form for every plane
MR2_FORCED = [(h, w, 2, 3, F16, 'aligned', (5, 0)) for (h, w) in [(45, 60), (21, 94), (61, 67)]]
REFUSED = [(2, 1204), (2, 1286)]


def case_id(c):
    return f'{c[0]}x{c[1]}-B{c[2]}C{c[3]}-{U.DT_NAME[c[4]]}-{c[5]}'


def run_case(lib, dev, c, tag=''):
    h, w, B, C, dtype, variant, route = c
    U.check_case(lib, dev, h, w, B, C, dtype, variant, route, tag)


@pytest.mark.parametrize('case', ALIGN_F32 + ALIGN_F16, ids=case_id)
def test_alignment_variants_emulated(case):
    run_case(emu_lib(), 'cpu', case)


@pytest.mark.parametrize('case', DFT_PRODUCTION, ids=case_id)
def test_dft_in_production_routing_emulated(case):
    run_case(emu_lib(), 'cpu', case)


@pytest.mark.parametrize('case', DFT_FORCED, ids=case_id)
def test_dft_forced_emulated(case, monkeypatch):
    monkeypatch.setenv('LAMA_FFT_MR', '0')
    run_case(emu_lib(), 'cpu', case, ' LAMA_FFT_MR=0')


@pytest.mark.parametrize('case', MR2_FORCED, ids=case_id)
def test_two_launch_mixed_radix_fp16_emulated(case, monkeypatch):
    monkeypatch.setenv('LAMA_FFT_MR', '2')
    run_case(emu_lib(), 'cpu', case, ' LAMA_FFT_MR=2')


@pytest.mark.parametrize('hw', REFUSED, ids=lambda s: f'{s[0]}x{s[1]}')
def test_refused_in_both_directions_emulated(hw):
    U.check_refused(emu_lib(), 'cpu', *hw)


def test_fourier_unit_refused_before_its_first_launch_emulated():
    U.check_fourier_unit_refused(emu_lib(), 'cpu')
