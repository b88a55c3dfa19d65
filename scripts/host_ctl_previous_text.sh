#!/bin/bash
# Writes the text the control-plane host-pointer calls had before they were staged through CtlStage (commit 14ecb1c:
# TmpDev, the argument checks, the twenty twins) to the file given, in the form tests/host_ctl_emulation.cpp takes with
# -DGPX_CTL_TEXT.  tests/golden/host_ctl_transcript.txt is that build's transcript:
#   scripts/host_ctl_previous_text.sh /tmp/previous.inc
#   g++ -std=c++20 -O1 -fsanitize=address,undefined -DGPX_CTL_TEXT='"/tmp/previous.inc"' -Iinclude -Igigapaxos_amd/csrc \
#       -o /tmp/previous tests/host_ctl_emulation.cpp && /tmp/previous --transcript-only > tests/golden/host_ctl_transcript.txt
# Needs that commit in the clone.  The line ranges are of the files as that commit has them; each is named below, and a
# range that cut a function in half would not compile.
set -euo pipefail
out=${1:?usage: $0 FILE}
rev=14ecb1c
C=gigapaxos_amd/csrc
cd "$(dirname "$0")/.."
lines() { git show "$rev:$C/$1" | sed -n "$2"; }
{
  # the copy macros of gpx_engine.hip, as they were
  echo '#define H2D_B(dst, src, bytes) HIPCHK(xfer(h, (dst), (src), (bytes), hipMemcpyHostToDevice, h->sB))'
  echo '#define D2H(dst, src, bytes) HIPCHK(xfer(h, (dst), (src), (bytes), hipMemcpyDeviceToHost, h->sB))'
  lines gpx_wire_host.inc '7,62p'; echo '}'          # "namespace {" and struct TmpDev
  echo 'extern "C" {'
  lines gpx_wire_host.inc '137,277p'                 # gpx_names_bind / unbind / lookup / coordinator, gpx_election_scan, gpx_gap_scan
  lines gpx_wire_host.inc '303,339p'                 # gpx_prepare_batch
  lines gpx_wire_host.inc '378,418p'                 # gpx_request_batch
  lines gpx_wire_host.inc '512,604p'                 # gpx_wire_decode
  lines gpx_wire_host.inc '679,834p'                 # gpx_wire_pack_accept_replies, gpx_wire_pack_commits
  lines gpx_elect_host.inc '49,108p'                 # gpx_election_begin, gpx_poke_scan
  lines gpx_elect_host.inc '151,211p'                # gpx_prepare_reply_batch
  echo '}'
  echo 'namespace {'
  lines gpx_scan_host.inc '29,48p'                   # scan_args, scan_lists
  lines gpx_scan_host.inc '70,97p'                   # scan_host
  lines gpx_sweep_host.inc '39,46p'                  # sweep_args
  echo '}'
  echo 'extern "C" {'
  lines gpx_scan_host.inc '146,192p'                 # gpx_election_scan_hits, gpx_poke_scan_hits, gpx_gap_scan_hits
  lines gpx_sweep_host.inc '75,109p'                 # gpx_pause_sweep
  echo '}'
  lines gpx_engine.hip '2216,2297p'; echo '}'        # 'extern "C" {', gpx_group_create, retire_impl, gpx_group_retire, gpx_group_snapshot
} > "$out"
