"""MI355X-native FM-SDR hot path (gfx950 HIP kernels behind a ctypes C-ABI).

Import with ``importlib.import_module("real-time-software-defined-radio_amd")`` (the
directory name is not an identifier) or ``import rtsdr`` from the repo root.

Drop-in per-block functions with the reference's names and signatures
(model/fmSupportLib.py, model/fmPll.py, model/fmRRC.py, scipy.signal.lfilter):

    lfilter, fmDemodArctan, fmPll, my_convoloution, impulseResponseRootRaisedCosine,
    my_filterImpulseResponse

fused hot-path forms: lfilter_decim, rf_frontend_block, mono_block, resample,
fm_mono_streams; the audio output stage (FM de-emphasis, int16 PCM): iir1, deemphasis, audio_out;
device-resident block pipelines: MonoBlockProcessor, StereoBlockProcessor,
RdsBlockProcessor; the wideband channelizer in front of a Receiver: Channelizer (any
frequencies) and FilterBank (a uniform grid of bins: the filter's work shared by all channels),
and RowResampler between them and the Receiver where fs / decim is not its 2.4 MS/s;
the RDS link layer behind the receiver's RRC rows: RdsLinkLayer (host, one stream) and
RdsLinkBank (device, every stream of a call), rds_groups; block synchronisation with a flywheel,
burst correction and offset C' behind it: RdsBlockSync (host, pure Python: the specification),
RdsSyncBank (device, RdsLinkBank.block_sync), and RdsProgramme (host: PI, PS name, radiotext from
the block records); symbol clock recovery in front of the block synchroniser, for receivers whose
crystal is off: RdsSymbolClock (host, pure Python: the specification) and RdsClockBank (device,
Receiver.rds_clock); carrier phase recovery in front of the clock, for stations, filters and PLL
settings that leave the RDS data off the in-phase row: RdsCarrierPhase (host, pure Python: the
specification) and RdsCarrierBank (device, Receiver.rds_carrier); the capture's spectrum / waterfall and the
station finder in front of them: Spectrum (device), find_channels (host); the spectrum of every
stream's demodulated row and the stereo / RDS indicators behind the receiver: RowSpectrum (device,
Receiver.mpx_spectrum), mpx_quality (host); the stereo blend and noise mute that act on that quality
on the device: BlendControl, BlendParams, audio_blend_dev, Receiver(blend=True); and in front of all of
the capture's stages, the correction of a direct-conversion front end's DC offset and IQ imbalance:
IqBalance (host, numpy f64: the specification) and IqCorrector (device); and in front of that, the
raw formats wideband front ends write (signed 8- and 16-bit IQ, narrower ADC codes in 16-bit words)
as the float32 capture, with a level meter of the ADC's codes: ingest_model, capture_format (host,
numpy: the specification) and CaptureIngest (device); and behind the receiver, the modulation
meter of its demodulated and audio rows (peak deviation, multiplex power, carrier offset, the
histogram of 50 ms peak holds): RowMeterModel, row_meter_model, modulation_report, mpx_levels (host,
numpy: the specification) and RowMeter (device, Receiver.modulation_meter, Receiver.audio_meter);
and on the audio rows, cascades of second-order sections (pilot notch, elliptic low-pass, DC
blocker, K-weighting) and the programme loudness of ITU-R BS.1770 built on them: sos_model,
LoudnessModel, loudness_report (host, numpy / scipy: the specification), RowSos
(Receiver.audio_filter) and LoudnessMeter (device, Receiver.loudness_meter); beside it the other two
figures of a broadcast monitor, the true peak of BS.1770 annex 2 and the loudness range of EBU Tech
3342: TruePeakModel, true_peak_report, loudness_range (host, numpy: the specification) and
TruePeakMeter (device, Receiver.true_peak_meter).
See DESIGN.md and INTEGRATION.md.
"""
from . import design, synth  # noqa: F401
from ._lib import (SDR_IQ_F32, SDR_IQ_S8, SDR_IQ_S16, SDR_IQ_U8, SDR_PRE_MIX, SDR_PRE_NONE, SDR_PRE_SQUARE, Context,  # noqa: F401
                   DeviceBuffer, SdrError, SdrUnavailable, Timer, device_count, device_info, get_context,
                   load_library)
from .blocks import (BlendControl, BlendParams, BlendState, CaptureIngest, Channelizer, FilterBank, IqCorrector, LoudnessMeter, MonoBlockProcessor, MpxQuality, RdsBlockProcessor, RdsCarrierBank, RdsClockBank, RdsLinkBank, RdsLinkLayer, RdsSyncBank,  # noqa: F401
                     Receiver, RowMeter, RowResampler, RowSos, RowSpectrum, Spectrum, StereoBlockProcessor, TruePeakMeter, find_channels, mpx_quality, rds_groups,
                     spectrum_rows)
from .rdssync import RdsBlockSync, RdsProgramme  # noqa: F401
from .rdsclock import RdsSymbolClock  # noqa: F401
from .rdscarrier import RdsCarrierPhase  # noqa: F401
from .iqbalance import IqBalance, IqState  # noqa: F401
from .capture import IngestMeter, capture_format, ingest_model  # noqa: F401
from .rowmeter import ModulationReport, MpxLevels, RowMeterModel, RowMeterRecord, modulation_report, mpx_levels, row_meter_model  # noqa: F401
from .sosfilter import LoudnessModel, LoudnessReport, loudness_report, sos_model  # noqa: F401
from .truepeak import LoudnessRange, TruePeakModel, TruePeakRecord, TruePeakReport, loudness_range, true_peak_report  # noqa: F401
from .design import impulseResponseRootRaisedCosine, my_filterImpulseResponse  # noqa: F401
from .dsp import (DFT, MonoState, estimatePSD, fm_mono_range, fm_mono_streams, split_halo, fmDemodArctan, fmPll, lfilter, lfilter_decim,  # noqa: F401
                  audio_blend_dev, audio_out, deemphasis, iir1, mono_block, my_convoloution, resample, rf_frontend_block)

__version__ = "0.1.0"
