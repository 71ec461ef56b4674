"""Float64 reference of the radar front end (rald_amd/csrc/radar_dsp.hip), shared by test_radar_dsp_ref.py and
test_gpu_radar_dsp_stages.py: plain numpy in complex128, written from the chain the kernel file's header and
tests/golden/make_golden_radar_dsp.py::margins describe.  Nothing here rounds to float32 or imitates the kernels' tiling, tables
or order of operations.

  frame_iq      int16 [ntx, nrx, nc, ns, 2] -> the mean-removed complex frame (what load_radar_data hands to RAEIVVmap)
  raeivv        complex [ntx, nrx, nc, ns] -> cube, range-Doppler map, decision margins, S and the noise level

The chain: Blackman window over the samples; fft(n=nr) over samples and fft(n=nd) over chirps (n shorter than the axis cuts, longer
pads), fftshift over Doppler; times exp(-2 pi i t (d - nd/2) / (ntx nd)) for the transmitter with data index t;
va[tel + rel, taz + raz] += rd[t, r]; fft(n=A) over azimuth, fftshift, fft(n=E) over elevation, fftshift; range bins
[0, int(nr crop_low)) and the last int(nr crop_high) zeroed; P = |.|^2; per (R, A, E) cell S = sum of P over Doppler,
vbins[argmax P], validity 0.7 top1 > top2; noise = quantile(S, 0.3) over the frame, dB = 10 log10(S / (noise + 1e-6) + 1)."""
import numpy as np

NOISE_Q = 0.30


def frame_iq(adc):
    """int16 [ntx, nrx, nc, ns, 2] -> complex128 [ntx, nrx, nc, ns] minus its complex mean over the whole frame"""
    adc = np.asarray(adc)
    x = adc[..., 0].astype(np.float64) + 1j * adc[..., 1].astype(np.float64)
    return x - np.mean(x)


def raeivv(x, tx, rx, vbins, nr, nd, A, E, crop_low, crop_high):
    """x complex [ntx, nrx, nc, ns] (used as given), tx / rx rows {data index, azimuth, elevation} ->
    dict(cube [nr, A, E, 3] float64 (dB, velocity, validity), rd [ntx * nrx, nr, nd] complex128 (channel = tx data index * nrx +
    rx data index; after the shift and the compensation), gap / thr [nr, A, E] ((top1 - top2) / top1 and |0.7 top1 - top2| / top1
    of the Doppler powers, 0 where top1 = 0), S [nr, A, E], noise)"""
    x = np.asarray(x, dtype=np.complex128)
    tx, rx = np.asarray(tx).reshape(-1, 3), np.asarray(rx).reshape(-1, 3)
    ntx, nrx, nc, ns = x.shape
    assert tx.shape[0] == ntx and rx.shape[0] == nrx
    x = x * np.blackman(ns).reshape(1, 1, 1, -1)
    d = np.fft.fftshift(np.fft.fft(np.fft.fft(x, nr, -1), nd, -2), -2)                    # (ntx, nrx, nd, nr)
    t = np.arange(ntx).reshape(-1, 1, 1, 1)
    k = (np.arange(nd) - nd // 2).reshape(1, 1, -1, 1)
    d = d * np.exp(-2j * np.pi * t * k / (ntx * nd))
    rd = d.reshape(ntx * nrx, nd, nr).transpose(0, 2, 1).copy()
    va = np.zeros((tx[:, 2].max() + rx[:, 2].max() + 1, tx[:, 1].max() + rx[:, 1].max() + 1, nd, nr), np.complex128)
    for tidx, taz, tel in tx:
        for ridx, raz, rel in rx:
            va[tel + rel, taz + raz] += d[tidx, ridx]
    e = np.fft.fftshift(np.fft.fft(np.fft.fftshift(np.fft.fft(va, A, 1), 1), E, 0), 0)    # (E, A, nd, nr)
    lo, hi = int(nr * crop_low), int(nr * crop_high)
    assert hi >= 1, "int(nr * crop_high) = 0 would zero every range bin (efft[..., -0:] = 0)"
    e[..., :lo] = 0
    e[..., nr - hi:] = 0
    P = (np.abs(e) ** 2).transpose(3, 1, 0, 2)                                             # (nr, A, E, nd)
    arg = np.argmax(P, axis=-1)
    srt = np.sort(P, axis=-1)
    top1, top2 = srt[..., -1], srt[..., -2]
    S = P.sum(-1)
    noise = float(np.quantile(S, NOISE_Q))
    cube = np.stack([10.0 * np.log10(S / (noise + 1e-6) + 1.0), np.asarray(vbins, np.float64)[arg],
                     (top1 * (1.0 - NOISE_Q) > top2).astype(np.float64)], axis=-1)
    den = np.where(top1 > 0, top1, 1.0)
    gap = np.where(top1 > 0, (top1 - top2) / den, 0.0)
    thr = np.where(top1 > 0, np.abs((1.0 - NOISE_Q) * top1 - top2) / den, 0.0)
    return dict(cube=cube, rd=rd, gap=gap, thr=thr, S=S, noise=noise)
