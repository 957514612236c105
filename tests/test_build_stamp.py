"""The source stamp (build.source_stamp) covers every file the library is compiled from: an edit to a
file it misses would leave a stale in-tree library that _lib.load() trusts."""
import os
import re

from raytracercuda_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _listed():
    return {os.path.normpath(os.path.join(build.CSRC, f)) for f in build.SOURCES + build.HEADERS}


def test_every_quoted_include_is_listed():
    listed = _listed()
    assert all(os.path.isfile(f) for f in listed)
    missing = []
    for f in sorted(listed):
        with open(f, encoding="utf-8", errors="replace") as fh:
            for inc in INCLUDE.findall(fh.read()):
                target = os.path.normpath(os.path.join(os.path.dirname(f), inc))
                if target not in listed:
                    missing.append(f"{os.path.relpath(f, build.REPO)} includes {inc}")
    assert not missing, f"not in SOURCES + HEADERS: {missing}"


def test_every_file_under_csrc_is_listed():
    listed = _listed()
    on_disk = {os.path.normpath(os.path.join(build.CSRC, f)) for f in os.listdir(build.CSRC)
               if f.endswith((".h", ".hip", ".cpp"))}
    assert on_disk <= listed, f"not in SOURCES + HEADERS: {sorted(os.path.basename(f) for f in on_disk - listed)}"
