"""``crop_to_mask`` with ``device_jpeg`` on two gloo ranks (emulated kernels), in the manner of tests/test_crop_gloo.py and tests/test_jpeg_gloo.py:
every rank runs the pre-pass and arrives at the same buckets, the one gather carries each rank's flat buffer of scans and lengths over
source-slot results, and the JPEGs rank 0 writes are those of the one-rank run, byte for byte -- also where a scan overflows its slot: the
fallback then runs a generator forward on rank 0 alone while the other rank waits in the reduction of the range flag, which must neither
deadlock nor change a file."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from lama_amd import predict as P
from tests import crop_util as U
from tests import jpeg_ref
from tests import step_matrix_util as M

JOIN_TIMEOUT = 600      # seconds for both workers together (they take about a minute): a deadlock fails the test instead of hanging it


def _kw():
    return dict(pad_mod=U.PAD_MOD, batch_size=1, device='cpu', io_threads=2, crop_to_mask=True, crop_margin=U.MARGIN, crop_step=U.STEP,
                out_ext='.jpg', device_jpeg=True)


def _worker(rank, world, port, indir, outdir, stride):
    import torch.distributed as dist
    from tests.test_dist_gloo import _build_model
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    P.JPEG_OUT_STRIDE = stride
    model = _build_model()[0]
    items = P.list_dataset(indir, '.png')
    n = P.predict(model, items, indir, outdir, rank=rank, world=world, dist=dist, **_kw())
    assert n == (len(items) if rank == 0 else 0)
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(port, indir, outdir, stride):
    """Both workers, joined within JOIN_TIMEOUT; what is still running then is killed and the test fails."""
    import time
    ctx = mp.spawn(_worker, args=(2, port, indir, outdir, stride), nprocs=2, join=False)
    deadline = time.monotonic() + JOIN_TIMEOUT
    try:
        while not ctx.join(timeout=5):                        # (raises if a worker failed)
            assert time.monotonic() < deadline, f'the two ranks did not finish within {JOIN_TIMEOUT} s'
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
                p.join()


@pytest.fixture(scope='module')
def one_rank(tmp_path_factory):
    """The pairs, the one-rank files with the default slots, and the scan lengths the overflowing run's slot size is chosen from."""
    from tests.test_dist_gloo import _build_model
    root = tmp_path_factory.mktemp('matrix_gloo')
    indir = str(root / 'in') + os.sep
    items = U.write_pairs(indir)        # batches of one: the 16 x 32 bucket gives rank 1 an empty round, the 16 x 16 bucket one image each
    model = _build_model()[0]
    out = str(root / 'one')
    assert P.predict(model, items, indir, out, **_kw()) == len(items)
    header = len(P.jpeg_from_scan(8, 8, 95, jpeg_ref.J420, b''))
    lens = {nm: os.path.getsize(os.path.join(out, nm)) - header for nm in M.files_of(out)}
    return dict(root=root, indir=indir, items=items, model=model, out=out, lens=lens)


def _same_files(a, b):
    names = M.files_of(a)
    assert names and names == M.files_of(b)
    for nm in names:
        with open(os.path.join(a, nm), 'rb') as fa, open(os.path.join(b, nm), 'rb') as fb:
            assert fa.read() == fb.read(), nm
    return names


def test_predict_world2_gloo_writes_the_one_rank_jpegs(one_rank, tmp_path):
    out2 = str(tmp_path / 'out2')
    _two_ranks(37500 + os.getpid() % 2000, one_rank['indir'], out2, None)
    assert len(_same_files(out2, one_rank['out'])) == 3


def test_predict_world2_gloo_with_a_scan_that_overflows(one_rank, tmp_path, monkeypatch):
    """Scan slots one byte shorter than the longest scan: that image alone overflows, on whichever rank computed it; rank 0 computes it again in
    the fallback's crop step and encodes it on the host -- the one-rank run's file of the same slot size, byte for byte -- while the other two
    files stay the device's."""
    lens = one_rank['lens']
    stride = max(lens.values()) - 1
    assert sorted(lens.values())[-2] <= stride, lens          # one scan overflows, no more
    out1, out2 = str(tmp_path / 'out1'), str(tmp_path / 'out2')
    monkeypatch.setattr(P, 'JPEG_OUT_STRIDE', stride)
    assert P.predict(one_rank['model'], one_rank['items'], one_rank['indir'], out1, **_kw()) == 3
    _two_ranks(38500 + os.getpid() % 2000, one_rank['indir'], out2, stride)
    names = _same_files(out2, out1)
    differs = []
    for nm in names:
        with open(os.path.join(out1, nm), 'rb') as f, open(os.path.join(one_rank['out'], nm), 'rb') as g:
            differs.append(f.read() != g.read())
    assert differs == [lens[nm] > stride for nm in names] and sum(differs) == 1          # the host's file for that image, the device's for the others
