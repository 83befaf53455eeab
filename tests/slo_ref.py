"""An independent reference for the sl stream (docs/OBJECTIVES.md): sorted() + bisect_right on the
finite samples.  It shares no code with apmbackend_amd."""
from bisect import bisect_right

ELAPSED_NAN = -2 ** 31


def thresholds(objectives, service):
    """The threshold list of a service under a gpu.latencyObjectives object."""
    named = (objectives or {}).get("services") or {}
    if service in named:
        return list(named[service])
    return list((objectives or {}).get("default") or [])


def window_counts(samples, thr):
    """(m, nan, [c_j]) of one window's samples (any order): c_j finite samples are <= thr[j]."""
    fin = sorted(v for v in samples if v != ELAPSED_NAN)
    return len(fin), len(samples) - len(fin), [bisect_right(fin, t) for t in thr]


def row(ts, server, service, samples, thr):
    """The sl row of a window, None without a threshold or without a finite sample."""
    m, nan, counts = window_counts(samples, thr)
    if m == 0 or not thr:
        return None
    pairs = ",".join("%d:%d" % (t, c) for t, c in zip(thr, counts))
    return f"sl|{ts}|{server}|{service}|{m}|{nan}|{pairs}"
