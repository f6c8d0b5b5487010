"""What every parent-bits fence shares.  A fence is a case module tests/<name>_cases.py (NAME, SOURCES and groups() ->
[(group id, keys, run)], run() -> {key: digest} in key order), a fixture tests/golden/<name>_bits.json that
tools/parent_bits.py wrote ONCE with the library of the commit before the fenced change, and a short test file that holds
the in-tree library to those digests.  Nothing here knows one case list."""
import hashlib
import json
import os
import re
import subprocess
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def digest(*tensors):
    """sha256 over the raw bytes of the tensors (host or device, made contiguous; NaN payloads included), in order,
    without a shape or dtype header."""
    import torch
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def load(name):
    """The parsed tests/golden/<name>_bits.json: library_commit, library, sha256 {key: digest}."""
    with open(os.path.join(ROOT, "tests", "golden", name + "_bits.json")) as f:
        return json.load(f)


def all_keys(cases):
    return [k for (_, keys, _) in cases.groups() for k in keys]


def all_digests(cases, progress=None):
    out = {}
    for (gid, keys, run) in cases.groups():
        got = run()
        assert list(got) == keys, gid
        out.update(got)
        if progress is not None:
            progress(gid, keys)
    return out


def _git(*args):
    try:
        return subprocess.run(("git", "-C", ROOT) + args, capture_output=True, text=True, timeout=30)
    except (OSError, subprocess.TimeoutExpired):
        return None


def assert_from_another_commit(fixture, sources):
    """The digests were not made by the library under test.  A fence proves that a change kept every output byte only if
    its digests come from the library BEFORE the change: a fixture regenerated with the in-tree library would agree with
    whatever that library computes.  So the fixture names the commit its library was built from, and that is another
    commit than HEAD -- or, in a work tree whose HEAD is still that commit, the kernel ``sources`` differ from it (paths
    that only the fixture's commit has count as different).  Without git, or outside a repository, only the format is
    checked."""
    commit = fixture["library_commit"]
    assert re.fullmatch(r"[0-9a-f]{40}", commit), commit
    head = _git("rev-parse", "HEAD")
    if head is not None and head.returncode == 0 and head.stdout.strip() == commit:
        diff = _git("diff", "--quiet", commit, "--", *sources)
        assert diff is not None and diff.returncode == 1, "the fixture was made by the library of this very commit"
    assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in fixture["sha256"].values())


def assert_keys(fixture, keys):
    """The fixture names exactly the launches ``keys`` of this tree, each once, in their order."""
    gold = fixture["sha256"]
    assert len(set(keys)) == len(keys)
    assert list(gold) == list(keys), (sorted(set(keys) - set(gold))[:5], sorted(set(gold) - set(keys))[:5])


def changed(got, gold, keys):
    """The keys whose digest is not the fixture's."""
    return [k for k in keys if got[k] != gold[k]]


def forced(pc, key, cfg, fn):
    """Run ``fn`` with the PackedConv ``pc`` pinned to the stored configuration ``cfg`` under ``key``; no fallback may
    happen: the key still holds it afterwards, nothing was added, no warning fired."""
    import torch
    pc.tuned.clear()
    pc.tuned[key] = tuple(cfg)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fn()
    torch.cuda.synchronize()
    assert dict(pc.tuned) == {key: tuple(cfg)} and not caught, (dict(pc.tuned), key, cfg, [str(w.message) for w in caught])
