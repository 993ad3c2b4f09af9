"""Records tests/golden/vocab_counts.json from the compiled reference (oracle/_ref/spm_encode, built by `make -C oracle ref`):
per (model, corpus) the lines `spm_encode --model=M --generate_vocabulary=true FILE` writes -- `piece TAB count`, by descending
count and then by piece -- and their md5.  The corpora: the first 600 lines of botchan.txt for every model, ja_sample.txt
for test_ja_model and (almost everything unknown) test_model.  tests/test_generate_vocabulary.py compares byte for byte.

    python scripts/make_vocab_golden.py
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


def corpora(model):
    botchan = open(os.path.join(GOLDEN, "botchan.txt"), "rb").read()
    out = {"botchan600": b"".join(botchan.splitlines(True)[:600])}
    if model in ("test_ja_model", "test_model"):
        out["ja"] = open(os.path.join(GOLDEN, "ja_sample.txt"), "rb").read()
    return out


def run(model, data, extra=()):
    with tempfile.NamedTemporaryFile(suffix=".txt") as f:
        f.write(data)
        f.flush()
        return subprocess.run([SPM_ENCODE, "--model=" + os.path.join(GOLDEN, model + ".model"), "--generate_vocabulary=true", *extra, f.name],
                              check=True, stdout=subprocess.PIPE, stdin=subprocess.DEVNULL, timeout=300).stdout


def main():
    if not os.path.exists(SPM_ENCODE):
        sys.exit("oracle/_ref/spm_encode is not built (make -C oracle ref)")
    out = {}
    for model in MODELS:
        out[model] = {}
        for name, data in corpora(model).items():
            image = run(model, data)
            lines = image.decode("utf-8", "surrogateescape").split("\n")
            assert lines.pop() == "", (model, name)
            out[model][name] = {"md5": hashlib.md5(image).hexdigest(), "lines": lines}
    with open(os.path.join(GOLDEN, "vocab_counts.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=True, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
