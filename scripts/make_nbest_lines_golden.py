"""Records tests/golden/nbest_lines.json from the compiled reference (oracle/_ref/spm_encode, built by `make -C oracle ref`):
what `spm_encode --output_format=nbest_id` and `--output_format=nbest_piece` write for botchan's first 200 lines at
`--nbest_size=3`, per model the md5 of the whole image, its size and its first 20 lines.  tests/test_encode_file_lattice.py
compares both md5s with what spmx_encode_file_ex writes for those formats.  (The reference's sample formats draw from a
thread-local mt19937 and cannot be pinned byte for byte.)

    python scripts/make_nbest_lines_golden.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SPM_ENCODE = os.path.join(ROOT, "oracle", "_ref", "spm_encode")
MODELS = ["test_model", "uni1k_bf"]
LINES, NBEST = 200, 3


def run(model, data, fmt):
    with tempfile.NamedTemporaryFile(suffix=".txt") as f:
        f.write(data)
        f.flush()
        return subprocess.run([SPM_ENCODE, "--model=" + os.path.join(GOLDEN, model + ".model"), "--output_format=" + fmt,
                               "--nbest_size=%d" % NBEST, f.name], check=True, stdout=subprocess.PIPE).stdout


def main():
    if not os.path.exists(SPM_ENCODE):
        sys.exit("oracle/_ref/spm_encode is not built (make -C oracle ref)")
    botchan = b"".join(open(os.path.join(GOLDEN, "botchan.txt"), "rb").read().splitlines(True)[:LINES])
    out = {"lines": LINES, "nbest_size": NBEST, "models": {}}
    for model in MODELS:
        out["models"][model] = {}
        for fmt in ("nbest_id", "nbest_piece"):
            image = run(model, botchan, fmt)
            out["models"][model][fmt] = {"md5": hashlib.md5(image).hexdigest(), "bytes": len(image),
                                         "head": image.decode("utf-8").split("\n")[:20]}
    with open(os.path.join(GOLDEN, "nbest_lines.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=True, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
