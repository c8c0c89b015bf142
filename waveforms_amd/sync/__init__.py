"""Receiver synchronisation (the reference has none): carrier phase and frequency recovery, ``carrier`` (``carrier_cpm`` for the
CPM detectors), and symbol timing recovery for SOQPSK-TG, ``timing``."""
