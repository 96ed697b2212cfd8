"""The sample rates at which the channelisers hand channels to the demodulators — shared by tests/test_channel_rates_golden.py,
tests/test_gpu_length_sweep.py (-m gpu), tests/test_abi_and_design.py and tools/make_goldens_channel_rates.py.  NumPy only.

pss_ddc, pss_pfb, pss_bank and pss_resample cut a 2.4 MS/s capture into channels of 37.5 .. 240 kS/s, and with exact_rate=True
formats.plan_audio resamples them to 22 050, 44 100 or 110 250 S/s: the decimation factors q = int(fs / 22050) are 1 .. 10 and
n_out = ceil((n - 1) / q) is nearly as long as the frame.  Each row: (rate, q, where a channel of that rate comes from).
"""
TARGET_RATE = 22050

NFM_RATES = [
    (37500.0, 1, "2.4 MS/s / 64"),
    (44100.0, 2, "plan_audio(rate, 'NFM')"),
    (48000.0, 2, "2.4 MS/s / 50 (the pss_ddc chain)"),
    (50000.0, 2, "2.4 MS/s / 48 (the 12.5 kHz band plan of pss_bank)"),
    (75000.0, 3, "2.4 MS/s / 32 (the pss_pfb chain)"),
    (110250.0, 5, "plan_audio's WFM rate fed to NFM"),
]
WFM_RATES = [
    (108000.0, 4, "the L - R band edge (53 kHz) at 0.98 of Nyquist"),
    (110250.0, 5, "plan_audio(rate, 'WFM')"),
    (120000.0, 5, "2.4 MS/s / 20"),
    (240000.0, 10, "2.4 MS/s / 10"),
]
SSB_RATES = [
    (22050.0, None, "plan_audio(rate, 'AM' / 'USB' / 'LSB' / 'RAW')"),
    (50000.0, None, "2.4 MS/s / 48"),
]
# what formats.plan_audio must return as rate_mid for these modes (test_channel_rates_golden checks it against the function)
PLAN_AUDIO = {"NFM": 44100.0, "WFM": 110250.0, "AM": 22050.0, "USB": 22050.0, "LSB": 22050.0, "RAW": 22050.0}

# rates at which the reference's SciPy calls raise ValueError: firwin's cutoff 15 kHz at or above Nyquist (NFM), butter's band edge 53 kHz
# at or above Nyquist (WFM)
NFM_REFUSED = [30000.0, 22050.0]
WFM_REFUSED = [106000.0]

# the frame lengths tests/golden/channel_rates.npz pins the oracle at: eleven of length_cases.GOLDEN_DEMOD_LENGTHS and 61, the shortest
# length at which n - 1 is a multiple of every q above (lcm(1, 2, 3, 4, 5, 10) = 60; no length of GOLDEN_DEMOD_LENGTHS has that property)
GOLDEN_LENGTHS = [29, 30, 61, 64, 129, 153, 256, 257, 1024, 1025, 2048, 2049]

# the product's own frame lengths: the chain tests', the default frame_len of demodulate_channels / demodulate_bank / monitor_channels,
# and one past NumPy's temporary-elision switch (n - 1) * 8 >= 262144 of the demodulators
PRODUCT_LENGTHS = [4096, 32768, 32770]
PRODUCT_NFM_RATES = [37500.0, 48000.0]
PRODUCT_WFM_RATES = [110250.0, 240000.0]


def factor(fs):
    return int(fs / TARGET_RATE)


def rate_id(fs):
    """37500.0 -> '37500_q1' (pytest ids)."""
    return f"{int(fs)}_q{factor(fs)}"
