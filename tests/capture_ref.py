"""Python twin of the capture loop (whisper_amd/host/captureLoop.h), written from the reference's text -- Capture::run, setStateFlag / clearStateFlag,
postPoolWork, CaptureParams and runCapture's checks of Whisper/Whisper/ContextImpl.capture.cpp -- and from the three departures the header documents
(end of stream, NoDrop, the Transcribing bit cleared by the loop's thread). Shared by tests/test_capture_cpu.py and tests/test_gpu_capture.py.

A run is a list of chunk sizes (one read each), a voice-activity answer per read, and a job script:
  vad(start, count) -> lastVoice   what detect answers for the buffer that begins at stream sample `start` and holds `count` samples
  job_passes[k]                    job k, posted in pass P of the loop, is found ended by a poll in pass >= P + job_passes[k] (a pass = one cancel check);
                                   waiting for a job always ends it
  cancel_at                        the pass whose cancel check answers "stop" (None: never)
run() returns dict(status=[words], pieces=[(start, end)], discarded=[(start, end)], passes=n)."""
import numpy as np

import vad_ref as V

LISTENING, VOICE, TRANSCRIBING, STALLED = 1, 2, 4, 0x80
STEREO, NO_DROP = 1, 2
FRAME = 256
f32 = np.float32


def samples_from_seconds(seconds):
    """:58-65 -- the product in float32, rounded to the nearest integer, ties to even"""
    return int(np.rint(f32(seconds) * f32(16000.0)))


class Params:
    def __init__(self, min_duration=2.0, max_duration=3.0, drop_start_silence=0.25, pause_duration=0.333, flags=0):
        self.seconds = (min_duration, max_duration, drop_start_silence, pause_duration)
        self.min, self.max, self.drop, self.pause = (samples_from_seconds(s) for s in self.seconds)
        self.flags = flags

    def valid(self):
        """:403-416"""
        return all(0.125 <= f32(s) <= 30.0 for s in self.seconds[:2])


def vad_from_intervals(intervals):
    """a scripted detector: frame f of a buffer that begins at `start` is speech when its first sample, start + 256 f, lies in one of the [a, b) intervals
    of stream samples. Less than one frame: 0 (voiceActivityDetection.cpp:124-129)."""
    def vad(start, count):
        last = 0
        for f in range(count // FRAME):
            s = start + FRAME * f
            if any(a <= s < b for a, b in intervals):
                last = (f + 1) * FRAME
        return last
    return vad


def vad_from_features(features_of):
    """the real detector: features_of(start, count) -> float32 [count // 256][3] of the buffered span, then the decision loop of tests/vad_ref.py"""
    def vad(start, count):
        if count // FRAME <= 0:
            return 0
        return V.decide(features_of(start, count))[1]
    return vad


def run(chunks, params, vad, job_passes=None, cancel_at=None):
    no_drop = bool(params.flags & NO_DROP)
    st = dict(word=0, size=0, start=0, next=0, last_voice=0, job_posted=None, jobs=0)
    status, pieces, discarded = [], [], []
    chunks = list(chunks)
    pos = [0]
    passes = [0]

    def set_flag(bit):
        old = st["word"]
        st["word"] |= bit
        if not old & bit:
            status.append(st["word"])

    def clear_flag(bit):
        old = st["word"]
        st["word"] &= ~bit
        if old & bit:
            status.append(st["word"])

    def job_length():
        k = st["jobs"] - 1
        return job_passes[k] if job_passes is not None and k < len(job_passes) else 0

    def post():
        # :134-147
        set_flag(TRANSCRIBING)
        pieces.append((st["start"], st["start"] + st["size"]))
        st["jobs"] += 1
        st["job_posted"] = passes[0]
        st["start"] = st["next"]
        st["size"] = 0
        st["last_voice"] = 0

    def wait_job():
        clear_flag(TRANSCRIBING)

    def read():
        if pos[0] >= len(chunks):
            return None
        n = chunks[pos[0]]
        pos[0] += 1
        return n

    def step():
        """one pass of Capture::run; False at the end of the stream"""
        if not no_drop and st["word"] & TRANSCRIBING and passes[0] >= st["job_posted"] + job_length():
            clear_flag(TRANSCRIBING)
        if st["word"] & STALLED:
            if st["word"] & TRANSCRIBING:
                n = read()                      # :221-222 discarded, the clock goes on
                if n is None:
                    return False
                discarded.append((st["next"], st["next"] + n))
                st["next"] += n
                return True
            clear_flag(STALLED)                 # :226-229
            post()
            return True
        old = st["size"]
        n = read()
        if n is None:
            return False
        st["size"] += n
        st["next"] += n
        new = st["size"]
        last = st["last_voice"] = vad(st["start"], new)
        if last == 0:                           # :238-249
            clear_flag(VOICE)
            if new < params.drop:
                return True
            st["size"] = 0
            st["start"] = st["next"]
            return True
        if last + params.pause >= old:          # :251-259
            set_flag(VOICE)
            if new < params.max:
                return True
        else:                                   # :260-266
            clear_flag(VOICE)
            if new < params.min:
                return True
        if not st["word"] & TRANSCRIBING:       # :270-276
            post()
            return True
        if no_drop:
            wait_job()
            post()
            return True
        if new < params.max:                    # :278-287
            return True
        set_flag(STALLED)
        return True

    set_flag(LISTENING)                         # :207
    ended = False
    while True:
        if cancel_at is not None and passes[0] == cancel_at:
            break
        more = step()
        passes[0] += 1
        if not more:
            ended = True
            break
    wait_job()
    if ended:
        clear_flag(STALLED)
        if st["size"] > 0 and st["last_voice"] != 0:
            post()
            wait_job()
    return dict(status=status, pieces=pieces, discarded=discarded, passes=passes[0])
