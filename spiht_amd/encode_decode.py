"""Command-line round trip of one image file on the GPU: `python -m spiht_amd.encode_decode IMAGE [--bpp 0.1 ...]`.

The argument schema is the reference tool's (encode_decode.py:17-26: same names, defaults and meaning), so a command
line written for it runs here; `--save FILE` additionally writes the encoding (utils.save_encoding) and `--load FILE`
decodes such a file instead of encoding IMAGE.  The body is organised as three steps -- plan (settings, level and bit
budget from the arguments and the picture), encode or load, decode and report -- each of which is usable on its own.
"""
import math
import time
from argparse import ArgumentParser
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .spiht_wrapper import (EncodingResult, SpihtSettings, decode_image, decode_image_reduced_u8, encode_image,
                            get_slices_and_h_w)
from .alloc import roi_map
from .rd import cut_to_psnr, rd_curve
from .tiles import (_codec_for, decode_image_layered, decode_image_layered_u8, decode_image_layered_window,
                    decode_image_layered_window_u8, decode_image_tiled, decode_image_tiled_u8, decode_image_window,
                    decode_image_window_u8, encode_image_layered, encode_image_tiled)
from .utils import imload, imsave, load_encoding, save_encoding

_ARGS = [  # (flag, type, default, help): the reference tool's options, then ours
    ("--bpp", float, 0.1, "bits per pixel"),
    ("--quantization_scale", float, 255.0, None),
    ("--level", int, None, "wavedec2 level. default is set so that the highest DWT level has a width and height of 4."),
    ("--wavelet", str, "bior2.2", "wavedec2 wavelet"),
    ("--mode", str, "reflect", "wavedec2 mode"),
    ("--color_model", str, "IPT", None),
    ("--per_channel_quant_scales", str, "1., 0.2, 0.2", None),
    ("--out", str, "reconstructed.png", "save reconstructed image to this file path"),
    ("--save", str, None, "also write the encoding to this file"),
    ("--load", str, None, "decode this encoding instead of encoding the image"),
    ("--reduce", int, 0, "decode at 1/2^K size (K pyramid levels below full size) and save that picture"),
    ("--psnr", float, None, "cut the stream to the shortest prefix found that reaches this PSNR in dB (of the float picture); with "
                            "--tile N --allocate rd: cut the tiles where the picture reaches it, --bpp the cap"),
    ("--rd-curve", int, None, "print N rows of the stream's rate-distortion curve: bytes, bpp, PSNR"),
    ("--tile", int, None, "code the picture as tiles of N x N, one stream per tile (the bit budget is shared equally)"),
    ("--window", str, None, "with --tile: decode only the window Y0,X0,H,W of the picture and save that (with --reduce K: of "
                            "the picture at 1/2^K size, in its coordinates)"),
    ("--allocate", str, None, "with --tile: 'rd' shares the bit budget between the tiles by their rate-distortion curves"),
    ("--points", int, 16, "with --allocate rd: prefixes measured per tile"),
    ("--layers", str, None, "with --tile N --allocate rd: Q quality layers, or their bit budgets b0,b1,... (the last one the "
                            "picture's); decodes after every layer"),
    ("--layer-psnr", str, None, "with --tile N --allocate rd: quality layers that reach the PSNRs DB0,DB1,... in dB (strictly "
                                "increasing), --bpp the cap; decodes after every layer"),
    ("--overlap", int, 0, "with --tile N: code every tile with a margin of M pixels of its neighbours (2 M <= N) and cross-fade the "
                          "decoded tiles over the 2 M pixels around each seam; goes with --window, --allocate rd and --layers"),
]


def build_parser():
    parser = ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("image_filename")
    for flag, typ, default, text in _ARGS:
        parser.add_argument(flag, type=typ, default=default, help=text)
    parser.add_argument("--roi", action="append", default=None, metavar="Y0,X0,H,W[:WEIGHT[:BACKGROUND]]",
                        help="with --tile N --allocate rd: a region of interest; the tiles share the bit budget by the squared "
                             "error weighted WEIGHT (255) inside the box and BACKGROUND (1) outside; repeatable, the larger "
                             "weight holds where regions overlap and the smallest background outside all of them")
    return parser


def roi_from_args(args, h, w):
    """--roi Y0,X0,H,W[:WEIGHT[:BACKGROUND]], once or several times -> the weight map uint8 [h, w], or None"""
    if not args.roi:
        return None
    if args.allocate != "rd":
        raise SystemExit("--roi needs --tile N --allocate rd")
    boxes, backgrounds = [], []
    for text in args.roi:
        parts = text.split(":")
        try:
            box = [int(v) for v in parts[0].split(",")]
            extra = [int(v) for v in parts[1:]]
        except ValueError:
            raise SystemExit("--roi %s: Y0,X0,H,W[:WEIGHT[:BACKGROUND]] in integers" % text)
        if len(box) != 4 or len(extra) > 2:
            raise SystemExit("--roi %s: Y0,X0,H,W[:WEIGHT[:BACKGROUND]]" % text)
        boxes.append(box + [extra[0] if extra else 255])
        backgrounds += extra[1:]
    try:
        return roi_map(h, w, boxes, background=min(backgrounds, default=1))
    except ValueError as e:
        raise SystemExit("--roi: %s" % e)


def default_level(h, w):
    """the deepest level that leaves the coarsest band at least 8 samples on its short side (encode_decode.py:33-38)"""
    return math.floor(min(math.log2(h / 8), math.log2(w / 8)))


@dataclass
class Plan:
    settings: SpihtSettings
    level: int
    max_bits: int


def plan(args, c, h, w) -> Plan:
    """what to code the c x h x w picture with.  A grey picture takes neither a colour model nor three channel
    scales (the reference's defaults would raise on it)."""
    scales = [float(v) for v in args.per_channel_quant_scales.split(",")]
    colour = c == 3
    return Plan(
        settings=SpihtSettings(wavelet=args.wavelet, quantization_scale=args.quantization_scale, mode=args.mode,
                               color_model=args.color_model if colour else None,
                               per_channel_quant_scales=scales if len(scales) == c else None),
        level=default_level(h, w) if args.level is None else args.level,
        max_bits=round(args.bpp * h * w))  # encode_decode.py:43


def timed(fn, *a):
    t0 = time.perf_counter()
    out = fn(*a)
    return out, time.perf_counter() - t0


def report_encoding(enc: EncodingResult, settings: SpihtSettings, seconds: Optional[float]):
    if seconds is not None:
        print("encoded in %.3f s: %.2f KiB" % (seconds, len(enc.encoded_bytes) / 1024))
    slices, _, _ = get_slices_and_h_w(enc.h, enc.w, settings, enc.level)
    print("  level %s, start plane %d, coarsest band %d x %d" % (enc.level, enc.max_n, slices[0][1].stop, slices[0][2].stop))


def main_tiled(args, picture):
    """--tile N [--window Y0,X0,H,W] [--reduce K]: the picture as tiles of N x N.  The level is a tile's (--level, or the default
    of an N x N picture); the bit budget of --bpp is shared equally among the tiles, or with --allocate rd [--points K] by
    their rate-distortion curves, which --roi Y0,X0,H,W[:WEIGHT[:BACKGROUND]] weights per pixel.  With --allocate rd, --psnr DB
    cuts the tiles where the picture reaches DB (weighted by --roi) with --bpp as the cap, and prints the bytes, the PSNR
    reached and whether the target was met.  --reduce K saves the 8-bit picture at 1/2^K size (the window in its coordinates)."""
    c, h, w = picture.shape
    if args.load or args.save or args.rd_curve is not None:
        raise SystemExit("--tile goes with --bpp, --level, the settings, --window, --reduce, --psnr and --out only")
    if (args.psnr is not None or args.layer_psnr is not None) and args.allocate != "rd":
        raise SystemExit("--psnr and --layer-psnr with --tile need --allocate rd")
    if args.psnr is not None and (args.layer_psnr is not None or args.layers is not None):
        raise SystemExit("--psnr is one rate; the layers' PSNRs are --layer-psnr DB0,DB1,...")
    if args.overlap and (args.roi or args.psnr is not None or args.layer_psnr is not None or args.reduce):
        raise SystemExit("--overlap goes with --window, --allocate rd and --layers; not with --roi, --psnr, --layer-psnr or --reduce")
    p = plan(args, c, h, w)
    # (the level is the coded tile's: with --overlap M a picture of N + 2 M)
    coded = args.tile + 2 * args.overlap
    level = default_level(coded, coded) if args.level is None else args.level
    print("encoding %d x %d x %d at %.3f bpp as tiles of %d x %d%s" % (c, h, w, args.bpp, args.tile, args.tile,
                                                                      ", overlap %d" % args.overlap if args.overlap else ""))
    roi = roi_from_args(args, h, w)
    if args.layers is not None or args.layer_psnr is not None:
        return main_layered(args, picture, p, level, roi)
    enc, secs = timed(lambda: encode_image_tiled(picture, args.tile, p.settings, level, p.max_bits, args.allocate, args.points,
                                                 roi=roi, target_psnr=args.psnr, overlap=args.overlap))
    gy, gx = enc.grid()
    print("encoded in %.3f s: %d x %d tiles, %.2f KiB" % (secs, gy, gx, len(enc.encoded_bytes) / 1024))
    if args.psnr is not None:
        # (the codec of the call above, which keeps its cut)
        cut = _codec_for(c, h, w, args.tile, p.settings, level, p.max_bits, np.float64, "rd", args.points).last_allocation
        print("cut to %.2f dB%s: %d bytes, %s" % (args.psnr, " (weighted by --roi)" if roi is not None else "",
                                                  len(enc.encoded_bytes), reached(cut)))
    if args.reduce:
        # the 8-bit picture of pyramid level K (no distance: there is no original of that size)
        if args.window:
            small, secs = timed(lambda: decode_image_window_u8(enc, p.settings, *_window(args), reduce=args.reduce))
        else:
            small, secs = timed(lambda: decode_image_tiled_u8(enc, p.settings, reduce=args.reduce))
        return enc, save_reduced(args, small, secs)
    if args.window:
        y0, x0, wh, ww = [int(v) for v in args.window.split(",")]
        decoded, secs = timed(decode_image_window, enc, p.settings, y0, x0, wh, ww)
        ref = picture[:, y0:y0 + wh, x0:x0 + ww]
        print("decoded the window %d x %d at (%d, %d) in %.3f s" % (wh, ww, y0, x0, secs))
    else:
        decoded, secs = timed(decode_image_tiled, enc, p.settings)
        ref = picture
        print("decoded in %.3f s" % secs)
    decoded = np.asarray(decoded)
    print("  mean squared error %.5f" % float(((ref - decoded) ** 2).mean()))
    imsave(args.out, decoded)
    print("  picture written to", args.out)
    return enc, decoded


def reached(cut):
    """what a TileAllocation of a call with a target PSNR says of it, in words"""
    if cut.met:
        return "PSNR %.3f dB, target met" % cut.psnr
    if cut.psnr is not None:
        return "PSNR %.3f dB with every tile's whole hull, target not reached" % cut.psnr
    return "the cut of the --bpp budget, target not reached within it"


def _window(args):
    return [int(v) for v in args.window.split(",")]


def save_reduced(args, small, secs):
    print("decoded %s at 1/%d size in %.3f s: %d x %d" % ("the window" if args.window else "the picture", 2 ** args.reduce, secs,
                                                          small.shape[1], small.shape[2]))
    imsave(args.out, small / 255)
    print("  picture written to", args.out)
    return small


def main_layered(args, picture, p, level, roi=None):
    """--layers Q | b0,b1,... or --layer-psnr DB0,DB1,...: the tiled picture in quality layers, given as bit budgets or as the
    PSNRs to reach under the cap of --bpp; the file is cut after every layer and decoded"""
    c, h, w = picture.shape
    if args.allocate != "rd":
        raise SystemExit("--layers and --layer-psnr need --tile N --allocate rd")
    layers, targets = None, None
    if args.layers is not None:
        layers = [int(v) for v in args.layers.split(",")]
        layers = layers[0] if len(layers) == 1 else layers
    if args.layer_psnr is not None:
        try:
            targets = [float(v) for v in args.layer_psnr.split(",")]
        except ValueError:
            raise SystemExit("--layer-psnr %s: DB0,DB1,... in dB" % args.layer_psnr)
    try:
        enc, secs = timed(lambda: encode_image_layered(picture, args.tile, p.settings, level, p.max_bits, layers, args.points,
                                                       roi=roi, target_psnr=targets, overlap=args.overlap))
    except ValueError as e:
        if targets is None:
            raise
        raise SystemExit("--layer-psnr: %s" % e)
    gy, gx = enc.grid()
    print("encoded in %.3f s: %d x %d tiles, %d layers, %.2f KiB" % (secs, gy, gx, enc.layers, len(enc.to_bytes()) / 1024))
    if targets is not None:
        cuts = _codec_for(c, h, w, args.tile, p.settings, level, p.max_bits, np.float64, "rd", args.points).last_allocation
        for q, (db, cut) in enumerate(zip(targets, cuts)):
            print("  layer %d to %.2f dB: %d bytes, %s" % (q, db, sum(cut.nbytes), reached(cut)))
    window = _window(args) if args.window else None
    if args.reduce:
        # every layer at 1/2^K size; the last one is saved
        for q, end in enumerate(enc.layer_ends()):
            if window is None:
                small, secs = timed(lambda: decode_image_layered_u8(enc, p.settings, q + 1, reduce=args.reduce))
            else:
                small, secs = timed(lambda: decode_image_layered_window_u8(enc, p.settings, *window, q + 1, reduce=args.reduce))
            print("  layer %d, %d file bytes" % (q, end))
        return enc, save_reduced(args, small, secs)
    ref = picture if window is None else picture[:, window[0]:window[0] + window[2], window[1]:window[1] + window[3]]
    print("  %6s %12s %10s" % ("layer", "file bytes", "PSNR dB"))
    for q, end in enumerate(enc.layer_ends()):
        if window is None:
            decoded = decode_image_layered(enc, p.settings, q + 1)
        else:
            decoded = decode_image_layered_window(enc, p.settings, *window, q + 1)
        mse = float(((ref - np.asarray(decoded)) ** 2).mean())
        print("  %6d %12d %10.3f" % (q, end, 10 * math.log10(1.0 / mse) if mse > 0 else math.inf))
    decoded = np.asarray(decoded)
    imsave(args.out, decoded)
    print("  picture written to", args.out)
    return enc, decoded


def main(args):
    picture = imload(args.image_filename)
    if args.tile is not None:
        return main_tiled(args, picture)
    if args.window or args.allocate or args.layers or args.roi or args.layer_psnr or args.overlap:
        raise SystemExit("--window, --allocate, --layers, --layer-psnr, --roi and --overlap need --tile")
    c, h, w = picture.shape
    p = plan(args, c, h, w)
    if args.load:
        enc, secs = load_encoding(args.load), None
    else:
        print("encoding %d x %d x %d at %.3f bpp" % (c, h, w, args.bpp))
        enc, secs = timed(encode_image, picture, p.settings, p.level, p.max_bits)
    report_encoding(enc, p.settings, secs)
    if args.rd_curve is not None:
        # (a loaded stream carries its own level: the one the decode below uses)
        curve, secs = timed(lambda: rd_curve(picture, p.settings, enc.level, result=enc, points=args.rd_curve))
        print("rate-distortion curve, %d prefixes in %.3f s" % (len(curve.byte_lengths), secs))
        print("  %10s %10s %10s" % ("bytes", "bpp", "PSNR dB"))
        for nbytes, bpp, db in zip(curve.byte_lengths, curve.bpp, curve.psnr):
            print("  %10d %10.4f %10.3f" % (nbytes, bpp, db))
    if args.psnr is not None:
        (enc, db, met), secs = timed(cut_to_psnr, picture, enc, args.psnr, p.settings)
        print("cut to %.2f dB in %.3f s: %d bytes, PSNR %.3f dB%s" % (args.psnr, secs, len(enc.encoded_bytes), db,
                                                                   "" if met else " (the whole stream: target not reached)"))
    if args.save:
        save_encoding(args.save, enc)
        print("  encoding written to", args.save)
    if args.reduce:
        # the 8-bit picture of pyramid level K, straight from the stream (no distance: there is no original of that size)
        small, secs = timed(decode_image_reduced_u8, enc, p.settings, args.reduce)
        print("decoded at 1/%d size in %.3f s: %d x %d" % (2 ** args.reduce, secs, small.shape[1], small.shape[2]))
        imsave(args.out, small / 255)
        print("  picture written to", args.out)
        return enc, small
    decoded, secs = timed(decode_image, enc, p.settings)
    decoded = np.asarray(decoded)[:, :h, :w]  # the inverse transform of an odd-sized picture is one sample longer
    print("decoded in %.3f s, mean squared error %.5f" % (secs, float(((picture - decoded) ** 2).mean())))
    imsave(args.out, decoded)
    print("  picture written to", args.out)
    return enc, decoded


if __name__ == "__main__":
    main(build_parser().parse_args())
