"""Texture mapping (include/rtc.h RTC_PAT_UV; the book's bonus chapter "Texture mapping", not in the reference).

A texture-mapped pattern maps its point to (u, v) -- planar, spherical, cylindrical or cube map, built with
:meth:`Pattern.texture_map` / :meth:`Pattern.cube_map` -- and hands it to a :class:`UvPattern`: UV checkers, an
align check, or an image :class:`Texture`.  The product library renders them on the device; the oracle restates the
reference, which has none, and refuses them.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, replace
from typing import Tuple, Union

import numpy as np

UV_MAPS = {"planar": 0, "spherical": 1, "cylindrical": 2, "cube": 3}
UV_KINDS = {"checkers": 0, "align_check": 1, "image": 2}
# image lookups (include/rtc.h RTC_UV_IMAGE*): nearest texel, or bilinear with the edge rule of each axis
UV_FILTERS = ("nearest", "linear")
UV_WRAPS = ("auto", "clamp", "u", "uv")
UV_LINEAR_KINDS = {"clamp": 3, "u": 4, "uv": 5}  # RTC_UV_IMAGE_LINEAR, _LINEAR_WRAP_U, _LINEAR_WRAP
UV_MAP_WRAPS = {"planar": "uv", "cylindrical": "uv", "spherical": "u", "cube": "clamp"}  # what wrap="auto" becomes under each map
MAX_SIDE = 16384  # include/rtc.h RTC_TEXTURE_MAX_SIDE


class Texture:
    """An image: ``rgb`` is an (h, w, 3) array of f64 colours, row 0 at the top.  Copied; compared by identity."""

    def __init__(self, rgb):
        a = np.array(rgb, dtype=np.float64, copy=True)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("Texture: rgb must have shape (height, width, 3), got %r" % (a.shape,))
        h, w = a.shape[0], a.shape[1]
        if h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE:
            raise ValueError("Texture: width and height must be 1 .. %d, got %d x %d" % (MAX_SIDE, w, h))
        self.rgb = np.ascontiguousarray(a)
        self.rgb.setflags(write=False)

    @property
    def width(self) -> int:
        return int(self.rgb.shape[1])

    @property
    def height(self) -> int:
        return int(self.rgb.shape[0])

    @staticmethod
    def from_ppm(src: Union[str, bytes, os.PathLike]) -> "Texture":
        """A texture from a PPM file (a path) or its bytes: P3 (the book's canvas_from_ppm: comments, free whitespace) or P6
        (8-bit, or 16-bit big-endian above maxval 255).  Values become value / maxval."""
        if isinstance(src, (bytes, bytearray, memoryview)):
            data = bytes(src)
        else:
            with open(src, "rb") as f:
                data = f.read()
        return Texture(read_ppm(data))


def read_ppm(data: bytes) -> np.ndarray:
    """(h, w, 3) f64 array of a P3 or P6 image, value / maxval.  Raises ValueError on a bad magic number, a truncated body or a
    maxval of 0 or above 65535."""
    pos = 0
    n = len(data)

    def token() -> bytes:
        nonlocal pos
        while pos < n:
            c = data[pos:pos + 1]
            if c == b"#":
                while pos < n and data[pos:pos + 1] not in (b"\n", b"\r"):
                    pos += 1
            elif c.isspace():
                pos += 1
            else:
                break
        start = pos
        while pos < n and not data[pos:pos + 1].isspace() and data[pos:pos + 1] != b"#":
            pos += 1
        if start == pos:
            raise ValueError("PPM: truncated header")
        return data[start:pos]

    def number(what: str) -> int:
        t = token()
        if not t.isdigit():
            raise ValueError("PPM: %s is not a number: %r" % (what, t))
        return int(t)

    magic = data[:2]
    if magic not in (b"P3", b"P6"):
        raise ValueError("PPM: bad magic number %r (P3 or P6 expected)" % (magic,))
    pos = 2
    w, h, maxval = number("width"), number("height"), number("maxval")
    if w < 1 or h < 1:
        raise ValueError("PPM: width and height must be at least 1")
    if maxval < 1 or maxval > 65535:
        raise ValueError("PPM: maxval must be 1 .. 65535, got %d" % maxval)
    count = w * h * 3
    if magic == b"P3":
        vals = []
        for _ in range(count):
            try:
                vals.append(number("sample"))
            except ValueError as e:
                if "truncated" in str(e):
                    raise ValueError("PPM: truncated body (%d of %d samples)" % (len(vals), count)) from None
                raise
        raw = np.array(vals, dtype=np.float64)
    else:
        if pos >= n or not data[pos:pos + 1].isspace():
            raise ValueError("PPM: truncated header")
        pos += 1  # the single whitespace byte before the raster
        size = 2 if maxval > 255 else 1
        body = data[pos:pos + count * size]
        if len(body) < count * size:
            raise ValueError("PPM: truncated body (%d of %d bytes)" % (len(body), count * size))
        raw = np.frombuffer(body, dtype=">u2" if size == 2 else np.uint8).astype(np.float64)
    return (raw / float(maxval)).reshape(h, w, 3)


@dataclass(frozen=True)
class UvPattern:
    """One UV pattern (include/rtc.h rtc_uv_pattern): what a texture map hands (u, v) to."""
    kind: str  # "checkers" | "align_check" | "image"
    width: float = 1.0
    height: float = 1.0
    texture: "Texture" = None
    children: Tuple = ()
    filter: str = "nearest"  # image: "nearest" | "linear" (bilinear)
    wrap: str = "auto"       # image, linear only: "clamp" | "u" | "uv" (the periodic axes), "auto" = what suits the map

    @staticmethod
    def checkers(width: float, height: float, a, b) -> "UvPattern":
        width, height = float(width), float(height)
        if not (math.isfinite(width) and width > 0.0 and math.isfinite(height) and height > 0.0):
            raise ValueError("UvPattern.checkers: width and height must be finite and > 0")
        return UvPattern("checkers", width, height, None, _patterns("checkers", (a, b)))

    @staticmethod
    def align_check(main, ul, ur, bl, br) -> "UvPattern":
        return UvPattern("align_check", children=_patterns("align_check", (main, ul, ur, bl, br)))

    @staticmethod
    def image(texture: Texture, filter: str = "nearest", wrap: str = "auto") -> "UvPattern":
        """An image lookup.  ``filter="linear"`` blends the four nearest texels; ``wrap`` says which axes are periodic there:
        ``"clamp"`` none (cube-map faces, decals), ``"u"`` u only (spherical maps), ``"uv"`` both (planar and cylindrical maps),
        ``"auto"`` the one that suits the map the pattern is put under.  ``filter="nearest"`` ignores ``wrap``."""
        if not isinstance(texture, Texture):
            raise TypeError("UvPattern.image: a Texture expected, got %s" % type(texture).__name__)
        if filter not in UV_FILTERS:
            raise ValueError("UvPattern.image: filter must be 'nearest' or 'linear', got %r" % (filter,))
        if wrap not in UV_WRAPS:
            raise ValueError("UvPattern.image: wrap must be 'auto', 'clamp', 'u' or 'uv', got %r" % (wrap,))
        return UvPattern("image", texture=texture, filter=filter, wrap=wrap)

    def resolved(self, mapping: str) -> "UvPattern":
        """This record under the map ``mapping``: a linear image's ``wrap="auto"`` becomes the map's own; anything else is itself."""
        if self.kind == "image" and self.filter == "linear" and self.wrap == "auto":
            return replace(self, wrap=UV_MAP_WRAPS[mapping])
        return self

    def kind_code(self, mapping: str = None) -> int:
        """The record's RTC_UV_* kind (include/rtc.h): 0..2, or 3..5 for a linear image."""
        if self.kind != "image" or self.filter == "nearest":
            return UV_KINDS[self.kind]
        if self.filter not in UV_FILTERS:
            raise ValueError("UvPattern: filter must be 'nearest' or 'linear', got %r" % (self.filter,))
        wrap = self.wrap
        if wrap == "auto":
            if mapping is None:
                raise ValueError("UvPattern: wrap='auto' is resolved by the map (Pattern.texture_map / Pattern.cube_map)")
            wrap = UV_MAP_WRAPS[mapping]
        if wrap not in UV_LINEAR_KINDS:
            raise ValueError("UvPattern: wrap must be 'auto', 'clamp', 'u' or 'uv', got %r" % (wrap,))
        return UV_LINEAR_KINDS[wrap]


def _patterns(what, kids) -> Tuple:
    from .scene import Pattern
    for k in kids:
        if not isinstance(k, Pattern):
            raise TypeError("UvPattern.%s: children must be Patterns, got %s" % (what, type(k).__name__))
    return tuple(kids)
