"""Command-line entry with the reference's invocation (python speech_enhancement_evaluator.py ENHANCEMENT_DIR
[PESQ_BIN_PATH]); see audio-visual-speech-enhancement_amd/speech_enhancement_evaluator.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avse_pkg  # noqa: E402

avse_pkg.load()
from avse_amd.speech_enhancement_evaluator import evaluate, main  # noqa: E402,F401

if __name__ == "__main__":
    main()
