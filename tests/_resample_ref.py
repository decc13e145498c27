"""Reference of the sample-rate conversion (dsmi_resample, csrc/resample.hip) in numpy, written from the definitions in
include/dsmi.h: ``ratecv`` is the closed form of ``audioop.ratecv(data, width, 1, rate_in, rate_out, None)`` in integer and
float64 arithmetic (exact), ``polyphase`` the direct sum y[j] = sum_k x[k] h[j down - k up] with the Kaiser-windowed sinc of
``scipy.signal.resample_poly``'s default design, together with the per-output quantities the error bound of the GPU test is
made of.  ``decode`` turns a WAV file's frames into the integers ``load_audio`` returns.  A helper module of the tests (not
collected)."""
import math

import numpy as np

WIDTH_DTYPE = {1: 3, 2: 0, 3: 4, 4: 5}      # sample width -> DSMI_PCM_{U8, I16, I24, I32}
PCM_STEREO = 16
POLYPHASE, RATECV = 0, 1


def decode(raw, width, channels=1):
    """Raw little-endian PCM frames -> int64 samples: the 8-bit bias of -128, two channels folded into their saturating sum."""
    buf = np.frombuffer(raw, dtype=np.uint8)
    if width == 1:
        x = buf.astype(np.int64) - 128
    elif width == 2:
        x = buf.view("<i2").astype(np.int64)
    elif width == 4:
        x = buf.view("<i4").astype(np.int64)
    else:
        a = buf.reshape(-1, 3).astype(np.int64)
        v = a[:, 0] | (a[:, 1] << 8) | (a[:, 2] << 16)
        x = np.where(v >= 1 << 23, v - (1 << 24), v)
    if channels == 2:
        lim = 1 << (8 * width - 1)
        x = np.clip(x[0::2] + x[1::2], -lim, lim - 1)
    return x


def encode(x, width):
    """int samples -> little-endian PCM frames of ``width`` bytes (8-bit: unsigned, biased by 128)."""
    x = np.asarray(x, dtype=np.int64)
    if width == 1:
        return (x + 128).astype(np.uint8).tobytes()
    if width == 2:
        return x.astype("<i2").tobytes()
    if width == 4:
        return x.astype("<i4").tobytes()
    u = (x & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], axis=1).astype(np.uint8).tobytes()


def ratio(rate_in, rate_out):
    g = math.gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g          # up (o), down (i)


def count(method, rate_in, rate_out, n):
    o, i = ratio(rate_in, rate_out)
    if n == 0:
        return 0
    return (n - 1) * o // i + 1 if method == RATECV else -((-n * o) // i)


def ratecv(x, width, rate_in, rate_out=16000):
    """``audioop.ratecv`` (weights 1, 0) of the int samples ``x`` of ``width`` bytes, as int64."""
    x = np.asarray(x, dtype=np.int64)
    o, i = ratio(rate_in, rate_out)
    n = len(x)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    sh = 32 - 8 * width
    X = x << sh
    j = np.arange((n - 1) * o // i + 1, dtype=np.int64)
    c = -((-j * i) // o)
    d = c * o - j * i
    prev = np.where(c > 0, X[np.maximum(c - 1, 0)], 0)
    v = prev.astype(np.float64) * d.astype(np.float64) + X[c].astype(np.float64) * (o - d).astype(np.float64)
    return np.trunc(v / np.float64(o)).astype(np.int64) >> sh


def as_reference_array(y, width):
    """Samples as the reference's ``AudioData.get_array_data`` returns them.  For 8-bit audio its ``_wav2array`` reads the
    bytes -- already biased by -128, i.e. signed -- as UNSIGNED, so what it returns is the signed sample modulo 256 (one to
    one on -128 .. 127); this package's 8-bit samples are the signed ones, as its ``load_audio`` has them.  Other widths: as is."""
    y = np.asarray(y, dtype=np.float64)
    return np.mod(y, 256.0) if width == 1 else y


def taps(rate_in, rate_out=16000):
    """(h[-half .. half], up, down): firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up."""
    up, down = ratio(rate_in, rate_out)
    mr = max(up, down)
    half = 10 * mr
    m = np.arange(-half, half + 1, dtype=np.float64)
    fc = 1.0 / mr                                         # firwin's own rounding: fc * sinc(fc * m), not sinc(m / mr) / mr -- where a
    h = fc * np.sinc(fc * m) * np.kaiser(2 * half + 1, 5.0)    # tap falls on a zero of the sinc its value IS the argument's rounding
    h *= up / h.sum()
    return h, up, down


def polyphase(x, rate_in, rate_out=16000, h=None):
    """(y, mag, K): y[j] = sum_k x[k] h[j down - k up] in float64 (numpy's dot per output), mag[j] = sum_k |x[k] h[...]| and
    K[j] = the number of taps output j meets inside the filter's support -- the terms of the GPU test's bound."""
    x = np.asarray(x, dtype=np.float64)
    up, down = ratio(rate_in, rate_out)
    if h is None:
        h = taps(rate_in, rate_out)[0]
    half = (len(h) - 1) // 2
    n = len(x)
    J = count(POLYPHASE, rate_in, rate_out, n)
    y, mag, K = np.zeros(J), np.zeros(J), np.zeros(J, dtype=np.int64)
    for j in range(J):
        k_hi = (j * down + half) // up
        k_lo = -((half - j * down) // up)                 # ceil((j down - half) / up)
        K[j] = k_hi - k_lo + 1
        k = np.arange(max(k_lo, 0), min(k_hi, n - 1) + 1)
        prod = x[k] * h[j * down - k * up + half]
        y[j] = prod.sum()
        mag[j] = np.abs(prod).sum()
    return y, mag, K


def resample(x, rate_in, method, width=None, rate_out=16000):
    """The float64 array ``dsmi_resample`` is held against: equal rates copy."""
    if rate_in == rate_out:
        return np.asarray(x, dtype=np.float64).copy()
    if method == RATECV:
        return ratecv(x, width, rate_in, rate_out).astype(np.float64)
    return polyphase(x, rate_in, rate_out)[0]
