"""Motion-JPEG in an AVI 1.0 container: complete JPEG files (what ``FrameSegmenter(encode='jpeg')`` returns) behind a RIFF
header, one file a player opens.  Host only, standard library only.

    RIFF <size> 'AVI '
      LIST <size> 'hdrl'
        'avih' 56   microseconds a frame, flags AVIF_HASINDEX, frames, 1 stream, the largest chunk, width, height
        LIST <size> 'strl'
          'strh' 56   'vids' 'MJPG', dwScale / dwRate = seconds a frame as a fraction, frames, the largest chunk
          'strf' 40   BITMAPINFOHEADER: width, height, 1 plane, 24 bits, compression 'MJPG', width * height * 3
      LIST <size> 'movi'
        '00dc' <length> file 0 [0 to an even length] '00dc' <length> file 1 ...
      'idx1' 16 a frame: '00dc', AVIIF_KEYFRAME, the chunk's offset from the 'movi' tag, its length

All integers little-endian.  A chunk's size field is the payload's length without the padding byte.  The header is written
with zeros for what is only known at the end (sizes, frame count, the largest chunk); ``close`` writes the index and patches
them.  ``AviReader`` reads such a file back: the JPEG payloads of the 'movi' list in order (the restart intervals of the
device encoder's files make them the decoder's multi-segment input).  AVI 1.0 sizes are 32 bits and players read them as signed: a write that would take the finished file past ``MAX_BYTES``
= 2^31 - 1 raises ``AviSizeError`` and leaves the file as it was (there is no OpenDML extension here).  No audio.
"""
import struct
from fractions import Fraction
from typing import List, Tuple

MAX_BYTES = 2 ** 31 - 1
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
_HDRL_BYTES = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))    # 'hdrl' avih LIST('strl' strh strf)
_MOVI_AT = 12 + 8 + _HDRL_BYTES                               # offset of the movi LIST's header
_INDEX_ENTRY = 16


class AviSizeError(ValueError):
    pass


class AviWriter:
    """``AviWriter(path, width, height, fps)``: ``write(jpeg_bytes)`` appends one frame, ``close()`` finishes the file;
    also a context manager.  The frames must be JPEG files of ``width`` x ``height`` (their SOI is checked, no more)."""

    def __init__(self, path, width: int, height: int, fps=25) -> None:
        width, height = int(width), int(height)
        if not (0 < width <= 65535 and 0 < height <= 65535):
            raise ValueError('AviWriter: width and height must be 1..65535, got {} x {}'.format(width, height))
        rate = Fraction(fps).limit_denominator(100000)
        if rate <= 0:
            raise ValueError('AviWriter: fps must be positive, got {!r}'.format(fps))
        self.width, self.height, self.fps = width, height, fps
        self._rate, self._scale = rate.numerator, rate.denominator
        self._index: List[Tuple[int, int]] = []    # (offset from the 'movi' tag, length) of every chunk
        self._largest = 0
        self._closed = False
        self._f = open(str(path), 'wb')
        self._f.write(self._header(0, 0))
        self._at = _MOVI_AT + 12                   # where the next chunk goes

    @property
    def frames(self) -> int:
        return len(self._index)

    def _header(self, riff_size: int, movi_size: int) -> bytes:
        n = len(self._index)
        avih = struct.pack('<14I', int(round(1e6 * self._scale / self._rate)), 0, 0, AVIF_HASINDEX, n, 0, 1, self._largest,
                           self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIiI4H', b'vids', b'MJPG', 0, 0, 0, 0, self._scale, self._rate, 0, n, self._largest, -1, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.width, self.height, 1, 24, b'MJPG', self.width * self.height * 3, 0, 0, 0, 0)
        strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
        hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
        assert len(avih) == 56 and len(strh) == 56 and len(strf) == 40 and len(hdrl) == _HDRL_BYTES
        return (b'RIFF' + struct.pack('<I', riff_size) + b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl
                + b'LIST' + struct.pack('<I', movi_size) + b'movi')

    def write(self, jpeg_bytes) -> None:
        if self._closed:
            raise ValueError('AviWriter.write: the file is closed')
        data = bytes(jpeg_bytes)
        if data[:2] != b'\xff\xd8':
            raise ValueError('AviWriter.write: not a JPEG file (no SOI marker in front)')
        padded = len(data) + (len(data) & 1)
        finished = self._at + 8 + padded + 8 + _INDEX_ENTRY * (len(self._index) + 1)
        if finished > MAX_BYTES:
            raise AviSizeError('AviWriter.write: frame {} of {} bytes would take the file to {} bytes, past the {} of AVI 1.0; '
                               'close this file and start another'.format(len(self._index), len(data), finished, MAX_BYTES))
        self._f.write(b'00dc' + struct.pack('<I', len(data)) + data + b'\x00' * (padded - len(data)))
        self._index.append((self._at - (_MOVI_AT + 8), len(data)))
        self._largest = max(self._largest, len(data))
        self._at += 8 + padded

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        try:
            idx = b''.join(struct.pack('<4sIII', b'00dc', AVIIF_KEYFRAME, at, n) for at, n in self._index)
            self._f.write(b'idx1' + struct.pack('<I', len(idx)) + idx)
            total = self._at + 8 + len(idx)
            self._f.seek(0)
            self._f.write(self._header(total - 8, self._at - (_MOVI_AT + 8)))
        finally:
            self._f.close()

    def __enter__(self) -> 'AviWriter':
        return self

    def __exit__(self, *exc) -> bool:
        self.close()
        return False


class AviReader:
    """``AviReader(path)``: iterates the JPEG payloads (``bytes``) of the 'movi' list of a file ``AviWriter`` wrote, in order;
    ``width``, ``height``, ``fps`` and ``len()`` come from the header.  ValueError on anything else: another header layout,
    another codec, a chunk that is not '00dc' or runs past the list, a frame count that disagrees with the header."""

    def __init__(self, path) -> None:
        with open(str(path), 'rb') as f:
            data = f.read()
        head = _MOVI_AT + 12
        if len(data) < head or data[:4] != b'RIFF' or data[8:12] != b'AVI ' or data[12:16] != b'LIST' \
                or data[20:28] != b'hdrlavih' or struct.unpack('<I', data[16:20])[0] != _HDRL_BYTES:
            raise ValueError('AviReader: {} is not an AVI file of the layout AviWriter writes'.format(path))
        avih = struct.unpack('<14I', data[32:88])
        strh_at = 88 + 12 + 8
        if data[88:92] != b'LIST' or data[96:104] != b'strlstrh' or data[strh_at:strh_at + 8] != b'vidsMJPG':
            raise ValueError('AviReader: {}: the stream is not Motion-JPEG video'.format(path))
        scale, rate = struct.unpack('<II', data[strh_at + 20:strh_at + 28])
        if data[_MOVI_AT:_MOVI_AT + 4] != b'LIST' or data[_MOVI_AT + 8:head] != b'movi' or scale == 0 or rate == 0:
            raise ValueError('AviReader: {}: no movi list where AviWriter puts it'.format(path))
        movi_size = struct.unpack('<I', data[_MOVI_AT + 4:_MOVI_AT + 8])[0]
        end = _MOVI_AT + 8 + movi_size
        if movi_size < 4 or end > len(data):
            raise ValueError('AviReader: {}: the movi list runs past the end of the file (not closed?)'.format(path))
        self.width, self.height = int(avih[8]), int(avih[9])
        self.fps = Fraction(rate, scale)
        self._frames: List[bytes] = []
        at = head
        while at < end:
            if at + 8 > end or data[at:at + 4] != b'00dc':
                raise ValueError('AviReader: {}: a chunk at {} that is not a video frame'.format(path, at))
            n = struct.unpack('<I', data[at + 4:at + 8])[0]
            if at + 8 + n > end:
                raise ValueError('AviReader: {}: the chunk at {} runs past the movi list'.format(path, at))
            self._frames.append(data[at + 8:at + 8 + n])
            at += 8 + n + (n & 1)
        if len(self._frames) != avih[4]:
            raise ValueError('AviReader: {}: {} frames in the movi list, {} in the header'.format(path, len(self._frames), avih[4]))

    def __len__(self) -> int:
        return len(self._frames)

    def __iter__(self):
        return iter(self._frames)

    def __getitem__(self, k: int) -> bytes:
        return self._frames[k]
