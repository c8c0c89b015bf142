"""Receiver synchronisation (the reference has none): carrier phase and frequency recovery, ``carrier`` (``carrier_cpm`` for the
CPM detectors), symbol timing recovery for SOQPSK-TG, ``timing`` (``timing_cpm`` for the CPM detectors), and both at once for
SOQPSK-TG, ``joint``."""
