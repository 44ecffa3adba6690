"""``crop_max_side`` on two gloo ranks (emulated kernels), in the manner of tests/test_crop_gloo.py: every rank runs the pre-pass and arrives at the
same buckets -- the shrunk windows in buckets of their own --, the one gather carries the source-slot result buffers, and the PNGs rank 0 writes
are those of the one-rank run, byte for byte."""
import os

import numpy as np
import torch
import torch.multiprocessing as mp

from lama_amd import predict as P
from tests import crop_shrink_util as U


def _worker(rank, world, port, indir, outdir):
    import torch.distributed as dist
    from tests.test_dist_gloo import _build_model
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    model = _build_model()[0]
    items = P.list_dataset(indir, '.png')
    n = P.predict(model, items, indir, outdir, pad_mod=U.PAD_MOD, batch_size=1, device='cpu', rank=rank, world=world, dist=dist, io_threads=2,
                  crop_to_mask=True, crop_margin=U.MARGIN, crop_step=U.STEP, crop_max_side=U.MAX_SIDE)
    assert n == (len(items) if rank == 0 else 0)
    dist.barrier()
    dist.destroy_process_group()


def test_predict_world2_gloo_writes_the_one_rank_pngs(tmp_path):
    from PIL import Image
    from tests.test_dist_gloo import _build_model
    indir = str(tmp_path / 'in') + os.sep
    items = U.write_pairs(indir)                      # batches of one: the shrunk 32 x 32 bucket gives each rank one image, the 16 x 32 bucket rank 1 an empty round
    out2, out1 = str(tmp_path / 'out2'), str(tmp_path / 'out1')
    port = 37500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, indir, out2), nprocs=2, join=True)
    model = _build_model()[0]
    assert P.predict(model, items, indir, out1, pad_mod=U.PAD_MOD, batch_size=1, device='cpu', crop_to_mask=True, crop_margin=U.MARGIN,
                     crop_step=U.STEP, crop_max_side=U.MAX_SIDE) == len(items)
    for j, (mask_path, img_path) in enumerate(items):
        rel = os.path.splitext(mask_path[len(indir):])[0] + '.png'
        with open(os.path.join(out2, rel), 'rb') as f2, open(os.path.join(out1, rel), 'rb') as f1:
            assert f2.read() == f1.read(), rel
        got = np.array(Image.open(os.path.join(out2, rel)))
        src, mask = np.array(Image.open(img_path).convert('RGB')), np.array(Image.open(mask_path).convert('L'))
        assert got.shape == src.shape == U.PAIRS[j][0] + (3,)
        assert np.array_equal(got[mask == 0], src[mask == 0]) and (got[mask != 0] != src[mask != 0]).any()
