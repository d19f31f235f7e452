#!/bin/bash
# tools/isa_diff.sh <tree A> <tree B>: device assembly of every imfnet_amd/csrc/*.hip of two checkouts, compared whole.
# Each file is compiled with its tree's Makefile FLAGS plus -S --cuda-device-only (no GPU needed, at most 16 jobs at a
# time); comment lines (;) and the .ident / .file lines are dropped, everything else -- every .amdhsa_* directive
# included -- must match.  Prints "<file>: <differing lines> of <lines>" and exits non-zero unless every count is 0.
# Extra compiler flags (an ablation switch, say) go in ISA_DIFF_FLAGS.
set -u
[ $# -eq 2 ] || { echo "usage: $0 <tree A> <tree B>" >&2; exit 2; }
export HIPCC=${HIPCC:-/opt/rocm/bin/hipcc} ARCH=${ARCH:-gfx950} ISA_DIFF_FLAGS=${ISA_DIFF_FLAGS:-}
export TMP_ISA=$(mktemp -d)
trap 'rm -rf "$TMP_ISA"' EXIT

listing() {   # <a|b> <tree> <file.hip>
  local dir=$2/imfnet_amd/csrc flags
  [ -f "$dir/$3" ] || { : > "$TMP_ISA/$1/$3.s"; return; }
  flags=$(sed -n 's/^FLAGS *:= *//p' "$dir/Makefile" | sed "s/\$(ARCH)/$ARCH/")
  (cd "$dir" && $HIPCC $flags $ISA_DIFF_FLAGS -S --cuda-device-only "$3" -o - 2> "$TMP_ISA/$1/$3.err") |
    grep -v -e '^[[:space:]]*;' -e '^[[:space:]]*\.ident' -e '^[[:space:]]*\.file' > "$TMP_ISA/$1/$3.s"
  [ -s "$TMP_ISA/$1/$3.s" ] || { echo "$2: $3 did not compile" >&2; cat "$TMP_ISA/$1/$3.err" >&2; }
}
export -f listing

mkdir "$TMP_ISA/a" "$TMP_ISA/b"
files=$( (cd "$1/imfnet_amd/csrc" && ls *.hip; cd "$2/imfnet_amd/csrc" && ls *.hip) | sort -u)
for f in $files; do printf '%s\n' a "$1" "$f" b "$2" "$f"; done | xargs -P 16 -n 3 -d '\n' bash -c 'listing "$@"' _

status=0
for f in $files; do
  n=$(diff "$TMP_ISA/a/$f.s" "$TMP_ISA/b/$f.s" | grep -c '^[<>]')
  lines=$(wc -l < "$TMP_ISA/a/$f.s")
  echo "$f: $n of $lines"
  [ "$n" -eq 0 ] && [ "$lines" -gt 0 ] || status=1
done
exit $status
