"""A 2-D gradient-echo image of a small synthetic phantom, acquired k-space sample by k-space sample.

    python examples/gre_imaging_2d.py [--plot]

The object is three tissues (T2 = 50, 70, 90 ms) with a proton-density map each on a 32 x 32 pixel lattice.  The state
matrix has ONE voxel per tissue; space enters through integer shifts (phase encoding, read-out steps) with
kvalue = 2 pi / FOV, and `epg.Imaging` sums, at every pixel, the phase states of every tissue weighted with the tissue's
density (`epg.System(weights=)`) and a box voxel, and adds everything up (`reduce=True`): one complex k-space sample per
acquisition, computed on the device.  An inverse FFT of the samples gives the image.

Checks printed at the end: the samples against the same acquisitions evaluated on the host (utils.imaging on the downloaded
state), and the reconstructed image against the phantom.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
from epgpy_amd import epg, utils  # noqa: E402

N, FOV = 32, 0.2                      # pixels per side, field of view (m)
T1, T2 = 1000.0, [50.0, 70.0, 90.0]
TE_STEP, TR = 0.05, 200.0             # ms between samples, repetition time

ax = (np.arange(N) - N // 2) * (FOV / N)
pixels = np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2)
x, y = pixels.T / FOV
r = np.hypot(x, y)
density = np.stack([np.where(r < 0.17, 1.0, 0.0),                                         # a disc
                    np.where((r >= 0.17) & (r < 0.30), 0.6 + 0.4 * x, 0.0),               # the ring around it, with a ramp
                    np.where((np.abs(x - 0.33) < 0.07) & (np.abs(y + 0.30) < 0.1), 0.8, 0.0)])   # a small rectangle


def sequence(sample):
    seq = [epg.System(weights=density, kvalue=2 * np.pi / FOV)]
    step, rest = epg.E(TE_STEP, T1, T2), epg.E(TR - N * TE_STEP, T1, T2)
    for line in range(N):
        seq += [epg.T(20, 0), epg.S([-(N // 2), line - N // 2])]       # excitation, prephasing + phase encoding
        seq += [sample, step, epg.S([1, 0])] * N                        # N samples, one read-out step apart
        seq += [epg.SPOILER, rest]
    return seq


options = dict(voxel_size=FOV / N, reduce=True)
samples = epg.simulate(sequence(epg.Imaging(pixels, **options)))                       # [N * N]
on_host = epg.simulate(sequence(epg.Probe(
    lambda sm: utils.imaging(pixels, sm.F, sm.k[..., :3], weights=density, **options))))
diff = float(np.max(np.abs(samples - on_host)))

# sample (line, i) sits at k = (i - N/2, line - N/2): the object is its inverse transform
kspace = samples.reshape(N, N).T                                                        # [kx, ky]
image = np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(kspace))) / N ** 2
phantom = density.sum(axis=0).reshape(N, N)
corr = float(np.corrcoef(np.abs(image).ravel(), phantom.ravel())[0, 1])

print(f"{N * N} acquisitions of {len(T2)} tissues x {N * N} pixels; |sample| at the centre of k-space: {abs(kspace[N // 2, N // 2]):.4f}")
print(f"largest difference to the acquisitions evaluated on the host: {diff:.2e}")
print(f"correlation of the reconstructed magnitude image with the phantom: {corr:.4f}")
for row in np.abs(image)[::2, ::2]:
    print("".join(" .:-=+*#%@"[min(int(9 * v / np.abs(image).max()), 9)] for v in row))
assert samples.shape == (N * N,) and diff < 1e-10 * np.abs(density).sum() and corr > 0.9

if "--plot" in sys.argv:
    import matplotlib.pyplot as plt
    fig, (left, right) = plt.subplots(1, 2)
    left.imshow(phantom), left.set_title("density"), right.imshow(np.abs(image)), right.set_title("|image|")
    plt.show()
