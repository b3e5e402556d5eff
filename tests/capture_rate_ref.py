"""numpy twin of the INDEX RULE of a live capture at another rate than 16 kHz (include/whisper_hip.h: wh_capture_create_rate), shared by
tests/test_capture_rate_cpu.py and tests/test_gpu_capture_rate.py. Written from the text of the rule, not from the kernel. It states which outputs of the
stream appear on which append / flush / skip and which input frames count as zero -- nothing else: sample values are never computed here, they are slices of
a whole-buffer resampling (resample_ref.resample on the CPU, wh_resample_host on the GPU) of the stream with those zeros in place, so they are exact by
construction.

With L, M, half, K of the rate (resample_ref.design), a stream holds n_in (input frames accepted), n_out (outputs emitted or skipped) and z (frames below it
read as zero):
    append( F )   n_in += F; the outputs [n_out, max( n_out, ready )) appear, ready = max( 0, ceil( ( n_in - half - 1 ) L / M ) )
    flush()       the outputs [n_out, ceil( n_in L / M )) appear; further appends are refused
    skip( F )     n_in += F; n_out = max( n_out, ceil( n_in L / M ) ); z = n_in; returns by how much n_out grew"""


def ceil_div(a, b):
    return -((-a) // b)


class Stream:
    def __init__(self, L, M, half, K):
        self.L, self.M, self.half, self.K = L, M, half, K
        self.n_in = self.n_out = self.z = 0
        self.flushed = False

    def ready(self, n_in):
        return max(0, ceil_div((n_in - self.half - 1) * self.L, self.M))

    def out_len(self, n_in):
        return ceil_div(n_in * self.L, self.M)

    def append(self, frames):
        """-> (first, last): the outputs [first, last) of the stream that this append puts into the buffer"""
        assert not self.flushed and frames >= 0
        self.n_in += frames
        first = self.n_out
        self.n_out = max(self.n_out, self.ready(self.n_in))
        return first, self.n_out

    def flush(self):
        assert not self.flushed
        self.flushed = True
        first = self.n_out
        self.n_out = max(self.n_out, self.out_len(self.n_in))
        return first, self.n_out

    def skip(self, frames):
        """-> by how much n_out grew: what the capture loop adds to its sample clock"""
        assert not self.flushed and frames >= 0
        self.n_in += frames
        grown = max(self.n_out, self.out_len(self.n_in)) - self.n_out
        self.n_out += grown
        self.z = self.n_in
        return grown

    def zeroed(self, x):
        """the stream as the filter sees it after the skips so far: a copy of x (frames on axis 0) with frames [0, z) set to zero"""
        y = x.copy()
        y[:self.z] = 0
        return y


def run(design, chunks):
    """chunks: ints (append), ("skip", F) or "flush" -> the list of output spans, one per entry, a skip's span being what it jumped over"""
    s = Stream(*design)
    spans = []
    for c in chunks:
        if c == "flush":
            spans.append(s.flush())
        elif isinstance(c, tuple):
            first = s.n_out
            s.skip(c[1])
            spans.append((first, s.n_out))
        else:
            spans.append(s.append(c))
    return s, spans
