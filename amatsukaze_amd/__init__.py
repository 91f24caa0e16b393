"""amatsukaze_amd -- MI355X-native logo / CM / KFM analysis hot path of nekopanda/Amatsukaze.

Product code only: HIP kernels + C ABI (csrc/, libamt_gpu.so) and the Python mirror of the reference's
filter interface (api.py).  Nothing here imports the CPU oracle.
"""
from .api import (DEINT_ADAPTIVE, DEINT_LINE, AMTAnalyzeLogo, AMTEraseLogo, AmtError, AmtsFile, AudioLevels, Context, Debander, DeviceClip, DeviceSurfaces, FrameStats, Logo, LogoCandidate, LogoFinder,
                  LogoFrame, LogoScan, Resizer, ScanLogo, ScanLogoAuto, ScanLogoAutoStream, ScanLogoFile, ScanLogoFileAuto, ScanLogoStream,
                  edge_level, extract_rect, kfm_render, kfm_render_plan, mute_sections, temporal_nr, weave_fields, write_chapter_exe)

__all__ = ["DEINT_ADAPTIVE", "DEINT_LINE", "AMTAnalyzeLogo", "AMTEraseLogo", "AmtError", "AmtsFile", "AudioLevels", "Context", "Debander", "DeviceClip", "DeviceSurfaces", "FrameStats", "Logo", "LogoCandidate",
           "LogoFinder", "LogoFrame", "LogoScan", "Resizer", "ScanLogo", "ScanLogoAuto", "ScanLogoAutoStream", "ScanLogoFile", "ScanLogoFileAuto",
           "ScanLogoStream", "edge_level", "extract_rect", "kfm_render", "kfm_render_plan", "mute_sections", "temporal_nr", "weave_fields", "write_chapter_exe"]
