"""The panadapter stage's host-side helpers (t41rx_set_panadapter; RxChain.set_panadapter): the firmware's constants and
the update-cadence rule the library's host code applies to every process call.  The colour table gradient[]
(Display.cpp:148-161) is the caller's: load it from wherever the application keeps it and hand it to
RxChain.set_panadapter_tables()."""

GRADIENT_WORDS = 117       # gradient[], Display.cpp:148-161
SPECTRUM_NOISE_FLOOR = 247  # spectrumNoiseFloor, gwv.cpp:18
UPDATE_PERIOD = 511        # ProcessIQData() calls per ShowSpectrum() sweep, one of them with updateDisplayFlag == 1 (Display.cpp:259-267)


def rows_of_call(counter, n_frames, period, phase):
    """The update frames of a process call of n_frames frames that starts at frame count `counter`: the frames f of the
    call, in order, with (counter + f) % period == phase.  Row k of the stage's buffers holds frame rows_of_call(..)[k].
    (rx_internal.hpp: pan_rows_of_call() is the same rule.)"""
    counter, n_frames, period, phase = int(counter), int(n_frames), int(period), int(phase)
    if period < 1 or not 0 <= phase < period or counter < 0 or n_frames < 0:
        raise ValueError("need period >= 1, 0 <= phase < period, counter >= 0, n_frames >= 0")
    first = (phase - counter) % period
    return list(range(first, n_frames, period))
