"""YUV4MPEG2 (Y4M) streams of 8-bit planar 4:2:0 frames, read and written in pure Python: what `ffmpeg -f yuv4mpegpipe`
exchanges over a pipe.

    YUV4MPEG2 W<width> H<height> F<num>:<den> I<p|t|b|m> A<num>:<den> C<colour space> X<comment> ...\\n
    FRAME[ parameters]\\n  <width * height + 2 * ((width + 1) // 2) * ((height + 1) // 2) bytes: Y, U, V planes>
    FRAME\\n ...

Accepted: C420jpeg, C420mpeg2, C420paldv, C420 and a missing C tag (= C420jpeg's layout), progressive or unstated
interlacing.  All of them are processed as centre-sited chroma; Header.siting_warning() is the line to print for the two
that are sited elsewhere.  Refused with a ValueError before a frame is read: C444, C422, C411, Cmono (with or without
alpha), any p10 / p12 / p14 / p16 depth, and interlaced material (It, Ib, Im)."""
from .image_utils import i420_frame_bytes

MAGIC = b"YUV4MPEG2"
ACCEPTED_CHROMA = ("420jpeg", "420mpeg2", "420paldv", "420")
SITED_ELSEWHERE = ("420mpeg2", "420paldv")
MAX_HEADER_BYTES = 4096


class Header:
    """The stream header.  width, height; fps, aspect: "num:den" strings or None; interlace: "p" or None; chroma: one of
    ACCEPTED_CHROMA or None (no C tag); comments: the X tags' values in order."""

    def __init__(self, width, height, fps=None, interlace=None, aspect=None, chroma=None, comments=()):
        self.width, self.height = int(width), int(height)
        self.fps, self.interlace, self.aspect, self.chroma = fps, interlace, aspect, chroma
        self.comments = tuple(comments)
        if self.width < 1 or self.height < 1:
            raise ValueError("larvanet_amd.y4m: a stream needs W and H >= 1, got %d x %d" % (self.width, self.height))
        if chroma is not None and chroma not in ACCEPTED_CHROMA:
            raise ValueError("larvanet_amd.y4m: colour space C%s is not supported: only 8-bit 4:2:0 (C420jpeg, C420mpeg2, "
                             "C420paldv, C420) is" % chroma)
        if interlace not in (None, "p"):
            raise ValueError("larvanet_amd.y4m: interlaced video (I%s) is not supported: deinterlace it first" % interlace)

    @property
    def frame_bytes(self):
        return i420_frame_bytes(self.width, self.height)

    @property
    def full_range(self):
        """True if an XCOLORRANGE=FULL comment is present, False for XCOLORRANGE=LIMITED, None if the stream does not say."""
        for c in self.comments:
            if c.upper().startswith("COLORRANGE="):
                return c.upper() == "COLORRANGE=FULL"
        return None

    def siting_warning(self):
        """The one line to print when the stream's chroma is not centre-sited, else None."""
        if self.chroma in SITED_ELSEWHERE:
            return ("WARNING: C%s chroma is sited left / co-sited; it is treated as centred (a shift of at most half a "
                    "chroma sample)" % self.chroma)
        return None

    def scaled(self, scale):
        """The header of the stream upscaled by `scale`: W and H multiplied, every other tag kept."""
        return Header(self.width * scale, self.height * scale, self.fps, self.interlace, self.aspect, self.chroma,
                      self.comments)

    def resized(self, width, height):
        """The header of the stream resized to width x height: W and H replaced, every other tag kept."""
        return Header(width, height, self.fps, self.interlace, self.aspect, self.chroma, self.comments)

    def to_bytes(self):
        tags = ["W%d" % self.width, "H%d" % self.height]
        tags += [t + v for t, v in (("F", self.fps), ("I", self.interlace), ("A", self.aspect), ("C", self.chroma))
                 if v is not None]
        tags += ["X" + c for c in self.comments]
        return MAGIC + b" " + " ".join(tags).encode("ascii") + b"\n"

    def __eq__(self, other):
        return isinstance(other, Header) and self.to_bytes() == other.to_bytes()

    def __repr__(self):
        return "Header(%s)" % self.to_bytes().decode("ascii").strip()


def parse_header(line):
    """The header line (bytes, with or without its newline) -> Header; ValueError for anything this package cannot
    process."""
    text = line.decode("ascii", errors="replace").rstrip("\n")
    fields = text.split(" ")
    if fields[0] != MAGIC.decode():
        raise ValueError("larvanet_amd.y4m: not a YUV4MPEG2 stream (it starts with %r)" % text[:16])
    width = height = fps = interlace = aspect = chroma = None
    comments = []
    for f in fields[1:]:
        if not f:
            continue
        tag, value = f[0], f[1:]
        if tag in "WH":
            if not value.isdigit():
                raise ValueError("larvanet_amd.y4m: bad %s tag %r" % (tag, f))
            if tag == "W":
                width = int(value)
            else:
                height = int(value)
        elif tag == "F":
            fps = value
        elif tag == "I":
            interlace = None if value == "?" else value
        elif tag == "A":
            aspect = value
        elif tag == "C":
            if value not in ACCEPTED_CHROMA:
                raise ValueError("larvanet_amd.y4m: colour space C%s is not supported: only 8-bit 4:2:0 (C420jpeg, "
                                 "C420mpeg2, C420paldv, C420) is" % value)
            chroma = value
        elif tag == "X":
            comments.append(value)
        else:
            raise ValueError("larvanet_amd.y4m: unknown header tag %r" % f)
    if width is None or height is None:
        raise ValueError("larvanet_amd.y4m: the header has no W or no H tag: %r" % text)
    return Header(width, height, fps, interlace, aspect, chroma, comments)


def _read_line(stream, limit, what):
    """Bytes up to and including the next newline; b"" at a clean end of the stream."""
    line = bytearray()
    while True:
        c = stream.read(1)
        if not c:
            if line:
                raise ValueError("larvanet_amd.y4m: the stream ends inside %s" % what)
            return b""
        line += c
        if c == b"\n":
            return bytes(line)
        if len(line) > limit:
            raise ValueError("larvanet_amd.y4m: %s is longer than %d bytes" % (what, limit))


def read_exact(stream, n):
    """Up to n bytes of a file or a pipe (a pipe returns short reads): fewer only at the end of the stream."""
    parts, got = [], 0
    while got < n:
        b = stream.read(n - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return b"".join(parts)


def read_header(stream):
    line = _read_line(stream, MAX_HEADER_BYTES, "the header")
    if not line:
        raise ValueError("larvanet_amd.y4m: the stream is empty")
    return parse_header(line)


def read_frames(stream, header):
    """Generator over the frames behind the header: bytes objects of header.frame_bytes.  ValueError naming the frame
    index for a frame that is cut short or does not start with FRAME."""
    import numpy as np
    n, index = header.frame_bytes, 0
    while True:
        line = _read_line(stream, MAX_HEADER_BYTES, "the FRAME line of frame %d" % index)
        if not line:
            return
        if line != b"FRAME\n" and not line.startswith(b"FRAME "):
            raise ValueError("larvanet_amd.y4m: frame %d does not start with FRAME but with %r" % (index, line[:16]))
        data = read_exact(stream, n)
        if len(data) != n:
            raise ValueError("larvanet_amd.y4m: frame %d is truncated: %d of %d bytes" % (index, len(data), n))
        yield np.frombuffer(data, dtype=np.uint8)
        index += 1


def read_raw_frames(stream, width, height):
    """Generator over the frames of a headerless .yuv stream of I420 frames; ValueError naming a truncated frame."""
    import numpy as np
    n, index = i420_frame_bytes(width, height), 0
    while True:
        data = read_exact(stream, n)
        if not data:
            return
        if len(data) != n:
            raise ValueError("larvanet_amd.y4m: frame %d is truncated: %d of %d bytes" % (index, len(data), n))
        yield np.frombuffer(data, dtype=np.uint8)
        index += 1


def write_header(stream, header):
    stream.write(header.to_bytes())


def write_frame(stream, frame):
    stream.write(b"FRAME\n")
    stream.write(memoryview(frame))
