"""GPU tests of constrained decoding through the host library and the command-line tool ("Constrained decoding") on the conditioned d = 128
model file, whose text tokens spell " w<id>": api.compile_phrases, Context.set_constraint, BatchRunner.set_constraint and whisper-main --allow-phrases agree."""
import subprocess
import wave

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_timestamp_rules as T  # noqa: E402  (its helpers: recordings, transcript keys)
from whisper_amd import api, build, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu
E_NOTIMPL = 0x80004001


def test_context_runner_and_tool_agree(tmp_path):
    """The phrase list = the words of the unconstrained transcripts but the commonest, joined by single spaces (repeat), penalty +inf. Context.run_full and a
    BatchRunner with two streams give the same transcripts, which differ from the unconstrained ones, hold text, and hold only listed words; whisper-main
    --allow-phrases FILE --allow-repeat --constraint-penalty inf writes the Context's transcript of the same file -- the C++ automaton against the Python one. --allow-repeat alone is
    refused. Beam search with a constraint held is E_NOTIMPL; off gives the unconstrained transcripts back."""
    path = str(tmp_path / "loop.bin")
    gf.write_model(path, gf.conditioned_model(gf.conditioned_layout(gf.hparams_for("test-d128-ml")), 4, kind="test-d128-ml", seed=4, alpha=30.0))
    model = api.Model(path)
    pcms = [np.clip(np.round(p * 32768.0), -32768, 32767).astype("<i2").astype(np.float32) / 32768.0 for p in (T._pcm(12, 250, 9), T._pcm(40, 330, 7))]
    kw = dict(language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT | api.SINGLE_SEGMENT)
    ctx, runner = model.create_context(), model.create_batch_runner(max_slots=2, groups=1)

    def both():
        out = []
        for pcm in pcms:
            assert ctx.run_full(pcm, **kw) == 0
            out.append(ctx.results())
        hr, got, per = runner.run(pcms, **kw)
        assert hr == 0 and all(p == 0 for p in per) and [T._key(g) for g in got] == [T._key(s) for s in out]
        return out

    plain = both()
    words = b" ".join(s["text"] for r in plain for s in r).split()
    allowed = sorted(set(words) - {max(set(words), key=words.count)})
    dfa = api.compile_phrases(allowed, repeat=True)
    ctx.set_constraint(*dfa, penalty=float("inf"))
    runner.set_constraint(*dfa, penalty=float("inf"))
    held = both()
    assert [T._key(h) for h in held] != [T._key(p) for p in plain]
    got_words = b" ".join(s["text"] for r in held for s in r).split()
    assert len(got_words) >= 1 and set(got_words) <= set(allowed)
    with pytest.raises(api.WhisperError) as e:
        ctx.run_full(pcms[0], beam_width=2, **kw)
    assert e.value.hr == E_NOTIMPL
    # the tool: a fresh context on the 16-bit file, default parameters
    wav, phrases = str(tmp_path / "rec.wav"), str(tmp_path / "phrases.txt")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.round(pcms[1] * 32768.0).astype("<i2").tobytes())
    open(phrases, "wb").write(b"\n".join(allowed) + b"\n")
    fresh = model.create_context()
    fresh.set_constraint(*dfa, penalty=float("inf"))
    assert fresh.run_full(pcms[1]) == 0
    texts = [s["text"] for s in fresh.results()]
    fresh.close()
    cmd = [build.CLI_BIN, "-m", path, "-f", wav, "-l", "en", "-nc"]
    r = subprocess.run(cmd + ["--allow-phrases", phrases, "--allow-repeat", "--constraint-penalty", "inf"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert [ln.split(b"]  ", 1)[1] for ln in r.stdout.splitlines() if b"]  " in ln] == texts and len(texts) >= 1
    assert subprocess.run(cmd + ["--allow-repeat"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300).returncode == 2
    ctx.set_constraint()
    runner.set_constraint()
    assert [T._key(b) for r in [both()] for b in r] == [T._key(p) for p in plain]
    runner.close()
    ctx.close()
    model.close()
