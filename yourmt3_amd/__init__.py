"""MI355X-native audio -> MIDI-token transcription path (see README.md / DESIGN.md).  Heavy imports are lazy so that
`import yourmt3_amd` works without a GPU or the built library."""

__all__ = ["YMT3Config", "YourMT3", "TaskManager", "transcribe", "score_notes", "evaluate", "note_metrics", "NoteMetrics", "piano_roll", "frame_metrics",
           "FrameMetricCounts", "PianoRoll", "baseline_config", "LiveTranscriber", "NoteStream", "dtw_align", "warp_notes", "Alignment", "Aligner",
           "align", "note_velocities", "NoteVelocity", "estimate_velocities", "track_beats", "beat_positions", "BeatTracker", "estimate_beats", "track_bars", "BarTracker", "estimate_bars", "track_chords", "ChordTracker", "estimate_chords", "track_sections", "SectionTracker", "estimate_sections", "split_hands", "HandSplitter", "estimate_hands"]


def __getattr__(name):
    if name in ("YMT3Config", "baseline_config"):
        from . import config
        return getattr(config, name)
    if name == "YourMT3":
        from .model import YourMT3
        return YourMT3
    if name == "TaskManager":
        from .task_manager import TaskManager
        return TaskManager
    if name == "transcribe":
        from .transcribe import transcribe
        return transcribe
    if name == "score_notes":
        from .transcribe import score_notes
        return score_notes
    if name == "evaluate":
        from .transcribe import evaluate
        return evaluate
    if name == "note_metrics":
        from .metrics import note_metrics
        return note_metrics
    if name == "NoteMetrics":
        from .model import NoteMetrics
        return NoteMetrics
    if name == "piano_roll":
        from .transcribe import piano_roll
        return piano_roll
    if name in ("frame_metrics", "FrameMetricCounts", "dtw_align", "warp_notes", "Alignment"):
        from . import metrics
        return getattr(metrics, name)
    if name == "LiveTranscriber":
        from .transcribe import LiveTranscriber
        return LiveTranscriber
    if name == "NoteStream":
        from .task_manager import NoteStream
        return NoteStream
    if name == "PianoRoll":
        from .model import PianoRoll
        return PianoRoll
    if name == "Aligner":
        from .model import Aligner
        return Aligner
    if name == "align":
        from .transcribe import align
        return align
    if name in ("note_velocities", "NoteVelocity", "estimate_velocities"):
        from . import velocity
        return getattr(velocity, name)
    if name in ("track_beats", "beat_positions", "BeatTracker", "estimate_beats"):
        from . import beats
        return getattr(beats, name)
    if name in ("track_bars", "BarTracker", "estimate_bars"):
        from . import bars
        return getattr(bars, name)
    if name in ("track_chords", "ChordTracker", "estimate_chords"):
        from . import chords
        return getattr(chords, name)
    if name in ("track_sections", "SectionTracker", "estimate_sections"):
        from . import sections
        return getattr(sections, name)
    if name in ("split_hands", "HandSplitter", "estimate_hands"):
        from . import hands
        return getattr(hands, name)
    raise AttributeError(name)
