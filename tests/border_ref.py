"""The border modes (include/srhip.h "Borders") restated in numpy: one np.pad per mode, and the crop as a slice.  Images are (n,H,W,C) or
(H,W,C) arrays of any dtype; nothing is converted."""
import numpy as np

NP_MODE = {"wrap": "wrap", "replicate": "edge", "mirror": "symmetric"}
MODES = tuple(NP_MODE)


def pad(img, mode, p):
    """The image continued by p pixels on every side of its two spatial axes."""
    img = np.asarray(img)
    lead = [(0, 0)] * (img.ndim - 3)
    return np.pad(img, lead + [(p, p), (p, p), (0, 0)], mode=NP_MODE[mode])


def crop(img, y0, x0, ch, cw):
    """The ch x cw window at (y0, x0), contiguous."""
    return np.ascontiguousarray(np.asarray(img)[..., y0:y0 + ch, x0:x0 + cw, :])


def centre(img, f, p):
    """What the composed calls cut out of the network's output for the padded image: the centre, f p pixels in from every side."""
    img = np.asarray(img)
    return crop(img, f * p, f * p, img.shape[-3] - 2 * f * p, img.shape[-2] - 2 * f * p)
