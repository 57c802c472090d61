#!/usr/bin/env python
"""Is a kernel file's device code the same in two revisions?  CPU only: it compiles, it opens no GPU.

    python tools/device_code_identity.py csrc/block.hip HEAD .
    python tools/device_code_identity.py csrc/block.hip HEAD~1 HEAD --flags-a=-DEM_BLOCK_FINE=1 --flags-b=-DEM_BLOCK_FINE=1

A side is a git revision, or a directory that holds a tree of this repository (`.`: the working tree).  The file and that
side's headers are copied to a temporary directory and compiled for the device alone with espnet_amd.build's flags; the
.text and .rodata sections and the `llvm-readelf --notes` dump (the kernel descriptors: VGPRs, LDS, scratch of every
instantiation) are hashed.  Exit status 1 if any of the three differs.  Bytes and metadata only: nothing is disassembled.
(Whole code objects are not compared: symbol tables and section offsets may differ where the code does not.)
"""
import argparse
import hashlib
import shlex
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from espnet_amd.build import EXTRA_FLAGS, FLAGS, HIPCC  # noqa: E402

LLVM = Path(HIPCC).resolve().parent.parent / "llvm" / "bin"
HEADER_DIRS = ["espnet_amd/csrc", "include"]


def checkout(side: str, rel: str, dst: Path) -> None:
    """The file `rel` and every header of `side` under dst, at their paths in the repository."""
    if Path(side).is_dir():
        tree = Path(side).resolve()
        files = [p.relative_to(tree) for d in HEADER_DIRS for p in (tree / d).iterdir() if p.suffix in (".h", ".inc")]
        for f in files + [Path(rel)]:
            (dst / f).parent.mkdir(parents=True, exist_ok=True)
            shutil.copyfile(tree / f, dst / f)
    else:
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", side, rel, *HEADER_DIRS], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", str(dst)], input=tar, check=True)


def hashes(side: str, rel: str, extra: list) -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        checkout(side, rel, tmp)
        obj = tmp / "device.o"
        # -cuid: hipcc names one symbol after a hash of the file's path and the flags, in hex WITHOUT leading zeros; one
        # time in sixteen the name is a character shorter, .rodata then starts 64 bytes earlier and every kernel
        # descriptor's offset to its code reads 64 more.  A fixed id gives both sides the same layout.
        cmd = [HIPCC, *FLAGS, *EXTRA_FLAGS.get(Path(rel).name, []), *extra, "--cuda-device-only", "--no-gpu-bundle-output",
               "-cuid=identity", "-c", str(tmp / rel), "-o", str(obj)]
        r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"hipcc failed for {side}:\n{r.stderr}")
        out = {}
        for sec in (".text", ".rodata"):
            raw = tmp / ("sec" + sec)
            subprocess.run([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=" + sec, str(obj), str(raw)], check=True)
            out[sec] = hashlib.sha256(raw.read_bytes()).hexdigest() + f" ({raw.stat().st_size} bytes)"
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(obj)], check=True, capture_output=True).stdout
        out["notes"] = hashlib.sha256(notes).hexdigest() + f" ({len(notes)} bytes)"
        return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("file", help="a file under espnet_amd/csrc, e.g. csrc/block.hip")
    ap.add_argument("a", help="git revision or tree directory")
    ap.add_argument("b", help="git revision or tree directory")
    ap.add_argument("--flags-a", default="", help="extra compiler flags of side a, e.g. --flags-a=-DEM_BLOCK_FINE=1")
    ap.add_argument("--flags-b", default="")
    args = ap.parse_args()
    rel = "espnet_amd/csrc/" + Path(args.file).name
    ha, hb = hashes(args.a, rel, shlex.split(args.flags_a)), hashes(args.b, rel, shlex.split(args.flags_b))
    same = True
    for key in ha:
        eq = ha[key] == hb[key]
        same &= eq
        print(f"{key:8s} a {ha[key]}\n{'':8s} b {hb[key]}  {'identical' if eq else 'DIFFERENT'}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
