"""Factory mirroring ``saicinpainting/training/modules/__init__.py:7-19``."""
import logging

from .ffc import FFCResNetGenerator
from .pix2pixhd import GlobalGenerator, MultiDilatedGlobalGenerator


def make_generator(config, kind, **kwargs):
    logging.info(f'Make generator {kind}')
    if kind == 'ffc_resnet':
        return FFCResNetGenerator(**kwargs)
    if kind == 'pix2pixhd_global':
        return GlobalGenerator(**kwargs)
    if kind == 'pix2pixhd_multidilated':
        return MultiDilatedGlobalGenerator(**kwargs)
    raise ValueError(f'Unknown generator kind {kind}')
