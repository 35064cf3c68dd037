"""TEST INFRASTRUCTURE — the reference for the window of a wind series' coming rows (include/wfseries.h), in NumPy.

The definition, as the header states it: a series of T rows (speed, direction); t ticks made since the series was set; farm b
starts at start[b].
  wind of farm b at tick u   series row (start[b] + u) % T, 0 <= u <= T - 1 (tick T does not exist)
  window (first, H)          entry h is the wind at tick min(t + first + h, T - 1), h = 0 .. H - 1
  available                  clamp(T - t - first, 0, H) entries are real; the rest hold the last tick's wind
tests/test_series.py pins this to the free wind the host env over the oracle observes over its next H steps."""
import numpy as np


def available(T, t, first, H):
    """clamp(T - t - first, 0, H)."""
    T, t, first, H = int(T), int(t), int(first), int(H)
    if T < 1 or not 0 <= t <= T - 1:
        raise ValueError("t must be a tick of the series: 0 .. T - 1")
    if first < 0 or H < 1:
        raise ValueError("first must be >= 0 and H >= 1")
    return min(max(T - t - first, 0), H)


def ticks(T, t, first, H):
    """(H,) the tick of every entry: min(t + first + h, T - 1)."""
    available(T, t, first, H)  # (the argument checks)
    return np.minimum(int(t) + int(first) + np.arange(int(H), dtype=np.int64), int(T) - 1)


def window(series, start, t, first, H, farms=None):
    """((n, H, 2) float64 — the rows themselves, no arithmetic —, available) of series (T, 2), start (B,) ints in [0, T) and
    farms (n,) indices into them (None: every farm)."""
    series = np.asarray(series, np.float64)
    if series.ndim != 2 or series.shape[1] != 2:
        raise ValueError("series must be (T, 2): speed, direction")
    T = series.shape[0]
    start = np.asarray(start, np.int64).reshape(-1)
    if ((start < 0) | (start >= T)).any():
        raise ValueError("a start row outside 0 .. T - 1")
    if farms is not None:
        start = start[np.asarray(farms, np.int64).reshape(-1)]
    rows = (start[:, None] + ticks(T, t, first, H)[None, :]) % T
    return series[rows], available(T, t, first, H)
