"""Records tests/golden/piece_lines.json from the compiled reference (oracle/_ref/spm_encode, built by `make -C oracle ref`):
per model the md5 of what `spm_encode --model=M < botchan.txt` writes with no format flag -- the piece-line image -- and
the piece lines of a handful of literal sentences.  tests/test_encode_pieces.py reads it for the models the oracle does not
restate (char1k, word1k) and for the pinned digest of test_model.

    python scripts/make_piece_lines_golden.py
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
MODELS = ["test_model", "uni1k_bf", "bpe1k_bf_uds", "bpe1k_llama", "test_ja_model", "char1k", "word1k"]
LINES = ["Hello world.", "", "   ", "I saw a girl with a telescope.", "the  quick   brown fox ", "zzqqxj 12345 éè",
         "吉祥寺で会いましょう", "Ｆｕｌｌ ①② ﬁ", "a"]


def run(model, data, extra=()):
    with tempfile.NamedTemporaryFile(suffix=".txt") as f:
        f.write(data)
        f.flush()
        return subprocess.run([SPM_ENCODE, "--model=" + os.path.join(GOLDEN, model + ".model"), *extra, f.name],
                              check=True, stdout=subprocess.PIPE).stdout


def main():
    if not os.path.exists(SPM_ENCODE):
        sys.exit("oracle/_ref/spm_encode is not built (make -C oracle ref)")
    botchan = open(os.path.join(GOLDEN, "botchan.txt"), "rb").read()
    literal = "".join(x + "\n" for x in LINES).encode("utf-8")
    out = {"lines": LINES, "models": {}}
    for model in MODELS:
        image = run(model, botchan)
        got = run(model, literal).decode("utf-8").split("\n")[:-1]
        assert len(got) == len(LINES), model
        out["models"][model] = {"botchan_md5": hashlib.md5(image).hexdigest(), "botchan_bytes": len(image),
                                "botchan300_md5": hashlib.md5(run(model, b"".join(botchan.splitlines(True)[:300]))).hexdigest(),
                                "pieces": got}
    with open(os.path.join(GOLDEN, "piece_lines.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=True, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
