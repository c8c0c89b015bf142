"""Receiver synchronisation (the reference has none): carrier phase and frequency recovery, ``carrier`` (``carrier_cpm`` for the
CPM detectors), symbol timing recovery for SOQPSK-TG, ``timing`` (``timing_cpm`` for the CPM detectors), both at once,
``joint`` (``joint_cpm``), and the coarse carrier frequency acquisition that brings an SOQPSK-TG burst into their range,
``coarse``."""
