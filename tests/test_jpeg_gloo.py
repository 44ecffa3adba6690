"""``device_jpeg`` on two gloo ranks (emulated kernels), in the manner of tests/test_png_gloo.py: the one gather carries each rank's flat buffer of
scans and lengths, and the JPEGs rank 0 writes are those of the one-rank run, byte for byte."""
import os

import numpy as np
import torch
import torch.multiprocessing as mp

from lama_amd import predict as P
from tests import paste_back_util as PB


def _worker(rank, world, port, indir, outdir):
    import torch.distributed as dist
    from tests.test_dist_gloo import _build_model
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    model = _build_model()[0]
    items = P.list_dataset(indir, '.png')
    n = P.predict(model, items, indir, outdir, pad_mod=8, batch_size=2, device='cpu', rank=rank, world=world, dist=dist, io_threads=2, out_ext='.jpg',
                  device_jpeg=True)
    assert n == (len(items) if rank == 0 else 0)
    dist.barrier()
    dist.destroy_process_group()


def test_predict_world2_gloo_writes_the_one_rank_jpegs(tmp_path):
    from PIL import Image
    from tests.test_dist_gloo import _build_model
    indir = str(tmp_path / 'in') + os.sep
    shapes = [(13, 16), (16, 11), (16, 16)]           # one bucket, batches of two: rank 0 gets two images, rank 1 one and an empty slot
    items = PB.write_pairs(indir, shapes)
    out2, out1 = str(tmp_path / 'out2'), str(tmp_path / 'out1')
    port = 36500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, indir, out2), nprocs=2, join=True)
    model = _build_model()[0]
    assert P.predict(model, items, indir, out1, pad_mod=8, batch_size=2, device='cpu', out_ext='.jpg', device_jpeg=True) == len(items)
    for j, (mask_path, img_path) in enumerate(items):
        rel = os.path.splitext(mask_path[len(indir):])[0] + '.jpg'
        with open(os.path.join(out2, rel), 'rb') as f2, open(os.path.join(out1, rel), 'rb') as f1:
            assert f2.read() == f1.read(), rel
        im = Image.open(os.path.join(out2, rel))
        assert np.array(im).shape == shapes[j] + (3,) and im.format == 'JPEG', rel
