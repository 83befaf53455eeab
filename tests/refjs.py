"""What the reference's own JavaScript answers to a request of tests/js/ref_harness.js.

The answers are stored under tests/golden/refjs/, one gzip-compressed JSON file per request,
named by the mode and the SHA-256 of the request text: the tests need neither node nor the
reference sources.  A request that differs in any byte from the recorded one (other synthetic
input, other oracle output fed into the next stage) has no file and fails the test.

To record again (the request changed on purpose), run the tests with ``APM_REF_RECORD=1`` and
``APM_REF_DIR`` naming a checkout of the reference; node executes its scripts through the harness.
"""
import gzip
import hashlib
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "js", "ref_harness.js")
GOLDEN = os.path.join(HERE, "golden", "refjs")


def _run_node(text: str) -> str:
    env = dict(os.environ, TZ="UTC")
    r = subprocess.run(["node", HARNESS], input=text, capture_output=True, text=True,
                       env=env, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-4000:])
    json.loads(r.stdout)
    return r.stdout


def _key(req: dict) -> str:
    """SHA-256 of the request; a config text counts without ``apmConfigFilePath``, the absolute
    path of the checkout's config file, which no answer depends on."""
    def bare(config_text):
        c = json.loads(config_text)
        c.pop("apmConfigFilePath", None)
        return json.dumps(c)
    r = dict(req)
    if "configText" in r:
        r["configText"] = bare(r["configText"])
    if "reloads" in r:
        r["reloads"] = [dict(x, configText=bare(x["configText"])) for x in r["reloads"]]
    return hashlib.sha256(json.dumps(r).encode("utf-8")).hexdigest()[:24]


def run(req: dict):
    text = json.dumps(req)
    path = os.path.join(GOLDEN, f"{req['mode']}_{_key(req)}.json.gz")
    if not os.path.exists(path):
        if not os.environ.get("APM_REF_RECORD"):
            raise RuntimeError(f"no recorded reference answer for this {req['mode']} request "
                               f"({os.path.basename(path)}): the request differs from the recorded one")
        out = _run_node(text)
        os.makedirs(GOLDEN, exist_ok=True)
        with open(path, "wb") as fh, gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
            gz.write(out.encode("utf-8"))
    with gzip.open(path, "rt", encoding="utf-8") as fh:
        return json.load(fh)


def parse(batch_list):
    req = {"mode": "parse",
           "batches": [{"now": now, "chunks": [[fp, ls] for fp, ls in chunks]} for now, chunks in batch_list]}
    return run(req)


def stats(lines):
    return run({"mode": "stats", "lines": lines})


def zscore(config_text, lines, reloads=()):
    """reloads: [(line index, config text)] applied as the reference's watcher does."""
    return run({"mode": "zscore", "configText": config_text, "lines": lines,
                "reloads": [{"at": a, "configText": t} for a, t in reloads]})


def alerts(config_text, lines, clock="entry", reloads=()):
    return run({"mode": "alerts", "configText": config_text, "lines": lines, "clock": clock,
                "reloads": [{"at": a, "configText": t} for a, t in reloads]})


def util(**kw):
    return run(dict(mode="util", **kw))
