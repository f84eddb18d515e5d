"""spiht_amd: MI355X-native drop-in for the hot path of theAdamColton/spiht.

Mirrors /root/reference/spiht/__init__.py:1-2: the wrapper API plus the two functions of the compiled
extension.  Importing the package loads libspiht_hip.so and fails loudly if it is absent.
"""
from . import _lib as _lib_mod

_lib_mod.lib()  # fail at import time, not at first use, when the HIP library has not been built

from .spiht_wrapper import (encode_image, decode_image, EncodingResult, SpihtSettings,  # noqa: E402,F401
                            ENCODER_DECODER_VERSION, encode_image_u8, decode_image_u8,
                            encode_image_u16, decode_image_u16, decode_image_reduced, decode_image_reduced_u8,
                            decode_image_reduced_u16, reduced_shape, decode_image_float, decode_image_reduced_float,
                            encode_image_float)
from . import floatpx  # noqa: E402,F401
from . import resample  # noqa: E402,F401
from .spiht import encode, decode  # noqa: E402,F401
from .rd import (RDCurve, rd_curve, rd_curve_u8, rd_curve_u16, cut_to_psnr, cut_to_psnr_u8,  # noqa: E402,F401
                 cut_to_psnr_u16)
from .tiles import (TiledCodec, TiledResult, TileCurves, TileAllocation, tile_grid, window_tiles, tiled_reduced_shape,  # noqa: E402,F401
                    encode_image_tiled, encode_image_tiled_u8, encode_image_tiled_u16, decode_image_tiled, decode_image_tiled_u8, decode_image_tiled_u16,
                    decode_image_window, decode_image_window_u8, decode_image_window_u16,
                    LayeredResult, encode_image_layered, encode_image_layered_u8, encode_image_layered_u16, decode_image_layered,
                    decode_image_layered_u8, decode_image_layered_u16, decode_image_layered_window, decode_image_layered_window_u8,
                    decode_image_layered_window_u16, decode_image_tiled_float, decode_image_window_float,
                    decode_image_layered_float, decode_image_layered_window_float, encode_image_tiled_float,
                    encode_image_layered_float)
from .alloc import roi_map, target_sqerr  # noqa: E402,F401
from .overlap import window_tiles_overlap  # noqa: E402,F401
from .hoststream import (StreamEncoder, StreamDecoder, StreamBusy, StreamTimeout, StreamIdle, encode_images,  # noqa: E402,F401
                         encode_images_u8, encode_images_u16, encode_images_float, decode_images, decode_images_u8,
                         decode_images_u16, decode_images_float)
from .tileset import TileSetCodec, cut_rule, paste_rule, set_tables  # noqa: E402,F401
