"""What the GPU tests ask the device itself."""
import functools
import subprocess
import sys


@functools.lru_cache(maxsize=None)
def device_cus():
    """Compute units of GPU 0 by torch.cuda.get_device_properties, read once per process in a fresh child: torch ships
    its own HIP runtime, and initialised after the library's in one process it was seen to find no GPU
    (tests/test_gpu_multi.py)."""
    code = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return int(p.stdout.split()[-1])
