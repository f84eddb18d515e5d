"""`import spiht` for callers written against the reference (its own scripts say `from spiht import encode_image`,
`from spiht.spiht_wrapper import SpihtSettings`, `from spiht.spiht import decode`, `from spiht.utils import imload`:
/root/reference/encode_decode.py:10-14, make_gif.py:9-12, demonstrate.py:10-13).

The package of this repository is `spiht_amd`; this one only re-exports it under the reference's name, module by
module, so an unchanged caller picks up the MI355X path.  Nothing is implemented here.
"""
import importlib
import sys

import spiht_amd as _impl

_SUBMODULES = ("spiht_wrapper", "spiht", "utils", "color_models", "spiht_py", "encode_decode", "rd", "tiles", "overlap", "floatpx",
               "hoststream")
for _name in _SUBMODULES:
    # `spiht.spiht` is the reference's compiled extension (src/lib.rs:58-65); here spiht_amd/spiht.py over the C ABI
    _mod = importlib.import_module("spiht_amd." + _name)
    sys.modules[__name__ + "." + _name] = _mod
    globals()[_name] = _mod
del _name, _mod

globals().update({_k: getattr(_impl, _k) for _k in ("encode_image", "decode_image", "EncodingResult", "SpihtSettings",
                                                    "ENCODER_DECODER_VERSION", "encode", "decode")})
# beyond the reference's names: the reduced-resolution decode
globals().update({_k: getattr(_impl, _k) for _k in ("decode_image_reduced", "decode_image_reduced_u8",
                                                    "decode_image_reduced_u16", "reduced_shape")})
# ... the rate-distortion curve of a stream and the cut to a target quality
globals().update({_k: getattr(_impl, _k) for _k in ("RDCurve", "rd_curve", "rd_curve_u8", "rd_curve_u16", "cut_to_psnr",
                                                    "cut_to_psnr_u8", "cut_to_psnr_u16")})
# ... tiled pictures: one stream per tile, parallel and windowed decode
globals().update({_k: getattr(_impl, _k) for _k in ("TiledCodec", "TiledResult", "tile_grid", "window_tiles",
                                                    "encode_image_tiled", "encode_image_tiled_u8", "encode_image_tiled_u16",
                                                    "decode_image_tiled", "decode_image_tiled_u8", "decode_image_tiled_u16",
                                                    "decode_image_window", "decode_image_window_u8",
                                                    "decode_image_window_u16")})
# ... quality layers of a tiled picture: any prefix of the file decodes
globals().update({_k: getattr(_impl, _k) for _k in ("LayeredResult", "encode_image_layered", "encode_image_layered_u8",
                                                    "encode_image_layered_u16", "decode_image_layered", "decode_image_layered_u8",
                                                    "decode_image_layered_u16", "decode_image_layered_window",
                                                    "decode_image_layered_window_u8", "decode_image_layered_window_u16")})
# ... tiled pictures at reduced resolution: the sizes of decode*(..., reduce=k)
globals().update({_k: getattr(_impl, _k) for _k in ("tiled_reduced_shape",)})
# ... region of interest: the weight map that the encode calls of tiled pictures take as roi=
globals().update({_k: getattr(_impl, _k) for _k in ("roi_map",)})
# ... target quality: the squared error that the encode calls' target_psnr= stands for
globals().update({_k: getattr(_impl, _k) for _k in ("target_sqerr",)})
# ... overlapping tiles: the tiles a window needs when the decoded tiles are cross-faded at the seams (the encode calls' overlap=)
globals().update({_k: getattr(_impl, _k) for _k in ("window_tiles_overlap",)})
# ... float pixels out: decodes into float32, float16 and bfloat16 pictures
globals().update({_k: getattr(_impl, _k) for _k in ("decode_image_float", "decode_image_reduced_float", "decode_image_tiled_float",
                                                    "decode_image_window_float", "decode_image_layered_float",
                                                    "decode_image_layered_window_float")})
# ... float pixels in: float32, float16 and bfloat16 pictures coded as they lie, by the float64 codec
globals().update({_k: getattr(_impl, _k) for _k in ("encode_image_float", "encode_image_tiled_float", "encode_image_layered_float")})
# ... host-fed streams: batches of host pictures encoded / streams decoded with the transfers overlapped
globals().update({_k: getattr(_impl, _k) for _k in ("StreamEncoder", "StreamDecoder", "StreamBusy", "StreamTimeout", "StreamIdle",
                                                    "encode_images", "encode_images_u8", "encode_images_u16",
                                                    "encode_images_float", "decode_images", "decode_images_u8",
                                                    "decode_images_u16", "decode_images_float")})
__all__ = ["encode_image", "decode_image", "EncodingResult", "SpihtSettings", "ENCODER_DECODER_VERSION", "encode", "decode"]
