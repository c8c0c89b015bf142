"""Receiver synchronisation (the reference has none): carrier phase and frequency recovery, ``carrier``."""
