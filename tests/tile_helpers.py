"""What the tiled GPU test files share: a device array of a host array, the padded picture and one tile's pixels, and the settings
and tile sides of a case."""
import numpy as np


def settings(cfg):
    import spiht_amd
    return spiht_amd.SpihtSettings(wavelet=cfg.get("wavelet", "bior2.2"), mode=cfg.get("mode", "reflect"),
                                   color_model=cfg.get("color"))


def tile_of(tile):
    return tuple(tile) if isinstance(tile, tuple) else (tile, tile)


def padded(P, th, tw):
    """the picture extended by edge replication to whole tiles"""
    H, W = P.shape[-2:]
    return np.pad(P, [(0, 0)] * (P.ndim - 2) + [(0, -H % th), (0, -W % tw)], mode="edge")


def tile_pixels(P, th, tw, i, j):
    return np.ascontiguousarray(padded(P, th, tw)[..., i * th:(i + 1) * th, j * tw:(j + 1) * tw])


def dev(arr):
    from spiht_amd import _lib
    from spiht_amd.batch import DeviceArray
    arr = np.ascontiguousarray(arr)
    d = DeviceArray(_lib.default_context(), arr.shape, arr.dtype)
    d.upload(arr)
    return d
