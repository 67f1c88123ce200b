"""SHA-256 of the .text section of every gfx950 code object in a built library, sorted -- the check that a host-only change left
the device code alone (the whole code object differs with any edit of a source file: hipcc derives a per-translation-unit id that
goes into symbol names from the source text).

    python tools/text_digests.py [path/to/libppyolo_hip.so] > digests.txt      # on both trees, then diff
"""
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'pytorch-ppyolo_amd'))
from ppyolo_hip import build  # noqa: E402


def text_digests(lib):
    objcopy = os.path.join(os.environ.get('ROCM_LLVM_BIN', '/opt/rocm/lib/llvm/bin'), 'llvm-objcopy')
    out = []
    with tempfile.TemporaryDirectory() as td:
        for i, co in enumerate(build.device_code_objects(lib)):
            src, txt = os.path.join(td, '%d.co' % i), os.path.join(td, '%d.text' % i)
            with open(src, 'wb') as fh:
                fh.write(co)
            subprocess.check_call([objcopy, '-O', 'binary', '--only-section=.text', src, txt])
            with open(txt, 'rb') as fh:
                data = fh.read()
            out.append('%s %8d' % (hashlib.sha256(data).hexdigest(), len(data)))
    return sorted(out)


if __name__ == '__main__':
    print('\n'.join(text_digests(sys.argv[1] if len(sys.argv) > 1 else build.LIB)))
