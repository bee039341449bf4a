"""`Image` — mirror of the reference's src/image.rs on the HIP backend.

`Image.par_render(camera, world)` is the reference's entry point of the hot path (src/image.rs:65-81); `read`, `write`,
`ppm` follow :83-112.  Quantisation (`Color::clamp`, src/color.rs:42-46) runs on the GPU, the P3 text is formatted by
the library's host code.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import cabi
from .scene import FUEL, Adaptive, Camera, Color, Filter, Sampling, Shutter, World


class Image:
    def __init__(self, hsize: int, vsize: int, pixels: np.ndarray = None, _native=None):  # src/image.rs:18-24
        self.hsize, self.vsize = int(hsize), int(vsize)
        self.pixels = np.zeros((self.vsize * self.hsize, 3), dtype=np.float64) if pixels is None else pixels
        self._native = _native  # (backend, NativeWorld) that rendered it, for the device quantiser

    @staticmethod
    def par_render(camera: Camera, world: World, fuel: int = FUEL, backend=None, sampling: Sampling = None, adaptive: Adaptive = None,
                   filter: Filter = None) -> "Image":
        """sampling: a :class:`Sampling` renders every pixel as the mean of its sample rays (anti-aliasing, depth of field); None is
        the reference's one ray per pixel.  adaptive: an :class:`Adaptive` renders the frame with its base sampling and only the pixels
        that differ from a neighbour with its fine one; it carries both samplings, so giving `sampling` as well is a ValueError.
        filter: a :class:`Filter` reconstructs every pixel from the samples within its radius instead of the pixel's own (without
        `sampling` that is one centre sample per pixel); the adaptive refine pass is not filtered, so `adaptive` with it is a ValueError."""
        if adaptive is not None and sampling is not None:
            raise ValueError("par_render: give `adaptive` or `sampling`, not both (an Adaptive carries its two samplings)")
        if adaptive is not None and filter is not None:
            raise ValueError("par_render: `filter` does not apply to `adaptive` (the refine pass is a box mean)")
        from . import hip_backend
        be = backend or hip_backend()
        nw = be.build_world(world)
        if adaptive is not None:
            return Image(camera.hsize, camera.vsize, be.render_adaptive(nw, camera, adaptive, fuel), (be, nw))
        if filter is not None:
            return Image(camera.hsize, camera.vsize, be.render_filtered(nw, camera, sampling if sampling is not None else Sampling(side=1), filter, fuel), (be, nw))
        if sampling is not None:
            return Image(camera.hsize, camera.vsize, be.render_sampled(nw, camera, sampling, fuel), (be, nw))
        rgb, _ = be.render(nw, camera, fuel, want_hits=False)
        return Image(camera.hsize, camera.vsize, rgb, (be, nw))

    @staticmethod
    def par_render_shutter(poses: Sequence[Tuple[Camera, World]], sampling: Sampling, shutter: Shutter = Shutter(), fuel: int = FUEL, backend=None) -> "Image":
        """Motion blur: `poses` are (camera, world) pairs over the shutter's opening, all cameras of one frame size; every sample of
        `sampling` is traced in the pose `shutter` deals it to and a pixel is the mean of its samples.  World objects that are the same
        object are built once and passed as one scene (a moving camera over a static world costs no memory)."""
        poses = list(poses)
        if not poses:
            raise ValueError("par_render_shutter: at least one pose")
        if not isinstance(sampling, Sampling) or not isinstance(shutter, Shutter):
            raise ValueError("par_render_shutter: `sampling` must be a Sampling and `shutter` a Shutter")
        for pose in poses:
            if not (isinstance(pose, tuple) and len(pose) == 2 and isinstance(pose[0], Camera) and isinstance(pose[1], World)):
                raise ValueError("par_render_shutter: every pose is a (Camera, World) pair")
        cam0 = poses[0][0]
        if any((c.hsize, c.vsize) != (cam0.hsize, cam0.vsize) for c, _ in poses):
            raise ValueError("par_render_shutter: the cameras' hsize or vsize differ")
        if not shutter.hashed and len(poses) > sampling.samples:
            raise ValueError("par_render_shutter: more poses than samples per pixel need Shutter(hashed=True)")
        from . import hip_backend
        be = backend or hip_backend()
        built = {}
        nws = []
        for _, world in poses:
            if id(world) not in built:
                built[id(world)] = be.build_world(world)
            nws.append(built[id(world)])
        rgb = be.render_shutter(nws, [c for c, _ in poses], sampling, shutter, fuel)
        return Image(cam0.hsize, cam0.vsize, rgb, (be, nws[0]))

    def _idx(self, x: int, y: int) -> int:  # :114-116
        return y * self.hsize + x

    def write(self, x: int, y: int, color: Color):  # :83-86
        self.pixels[self._idx(x, y)] = (color.r, color.g, color.b)

    def read(self, x: int, y: int) -> Color:  # :88-91
        r, g, b = self.pixels[self._idx(x, y)]
        return Color(float(r), float(g), float(b))

    def _lib_and_scene(self):
        from . import hip_backend
        from .scene import World as _W
        if self._native is None:
            be = hip_backend()
            self._native = (be, be.build_world(_W([], [])))
        be, nw = self._native
        scene = be._lib.rtw_world_scene(nw.handle, 0)
        if not scene:
            raise RuntimeError("scene upload failed: %s" % be._err())
        return be._lib, scene

    def quantized(self) -> np.ndarray:
        """Color::clamp of every channel, on the GPU: (vsize*hsize, 3) uint8."""
        lib, scene = self._lib_and_scene()
        src = np.ascontiguousarray(self.pixels, dtype=np.float64)
        out = np.empty(src.shape, dtype=np.uint8)
        if lib.rtc_quantize(scene, src.ctypes.data, src.size, out.ctypes.data) != 0:
            raise RuntimeError("rtc_quantize: %s" % (lib.rtc_last_error() or b"").decode())
        return out

    def ppm(self) -> str:  # :93-112
        return ppm_text(self.hsize, self.vsize, self.quantized())


def ppm_text(hsize: int, vsize: int, rgb8: np.ndarray, lib=None) -> str:
    """Image::ppm layout from quantised pixels (host-side formatting in librtc_amd.so; needs no GPU)."""
    if lib is None:
        from . import _LIB
        lib = cabi.load(_LIB)
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    assert rgb8.size == hsize * vsize * 3
    need = lib.rtc_ppm(hsize, vsize, rgb8.ctypes.data, None, 0)
    buf = C.create_string_buffer(int(need) + 1)
    lib.rtc_ppm(hsize, vsize, rgb8.ctypes.data, buf, need + 1)
    return buf.value.decode()
