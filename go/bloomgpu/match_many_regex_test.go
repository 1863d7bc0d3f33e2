package bloomgpu

import "testing"

// MatchRowsManyRegex: two queries sharing one FieldRegex condition in one call; every plane equals MatchRowsRegex for its query
// alone, a set's mask switches a query off on that set's rows, and a pattern outside the device's subset answers IsUnsupported.
// Needs a gfx950 device; skipped otherwise.
func TestMatchRowsManyRegex(t *testing.T) {
	g, err := Open([]int32{0})
	if err != nil {
		t.Skip(err)
	}
	defer g.Close()
	var rows []byte
	off := []uint64{0}
	for _, r := range []string{`{"level":"error","service":"payment"}`, `{"level":"info","service":"payment"}`, `{"level":"error","service":"auth"}`} {
		rows = append(rows, r...)
		off = append(off, uint64(len(rows)))
	}
	// table: 0 = FieldToken(level, error), 1 = FieldRegex(service, ^pay); query 0 = And(0, 1), query 1 = And(TRUE, 1)
	conds := []MatchCond{{Kind: KindFieldToken, Field: "level", Token: "error"}, {Kind: KindFieldRegex, Field: "service", Token: "^pay"}}
	progOps := []uint32{OpTerm<<28 | 0, OpTerm<<28 | 1, OpAnd<<28 | 2, OpTrue << 28, OpTerm<<28 | 1, OpAnd<<28 | 2}
	progOff := []uint32{0, 3, 6}
	planes, host, err := g.MatchRowsManyRegex(rows, off, conds, progOps, progOff, nil, nil, nil)
	if err != nil || len(host) != 0 || len(planes) != 2 {
		t.Fatalf("planes %v host %v err %v", planes, host, err)
	}
	if planes[0][0] != 0b001 || planes[1][0] != 0b011 {
		t.Fatalf("planes %v", planes)
	}
	for q := 0; q < 2; q++ {
		one, _, err := g.MatchRowsRegex(rows, off, conds, progOps[progOff[q]:progOff[q+1]])
		if err != nil || one[0] != planes[q][0] {
			t.Fatalf("query %d: single call %v err %v, plane %v", q, one, err, planes[q])
		}
	}
	// two sets: rows {0, 1} evaluate query 0 only, row {2} query 1 only
	planes, host, err = g.MatchRowsManyRegex(rows, off, conds, progOps, progOff, []uint32{0, 2, 3}, []uint64{0b01, 0b10}, nil)
	if err != nil || len(host) != 0 {
		t.Fatalf("masked: host %v err %v", host, err)
	}
	if planes[0][0] != 0b001 || planes[1][0] != 0 {
		t.Fatalf("masked planes %v", planes)
	}
	// a pattern outside the device's subset
	_, _, err = g.MatchRowsManyRegex(rows, off, []MatchCond{{Kind: KindFieldRegex, Field: "level", Token: `\bx`}}, []uint32{OpTerm << 28}, []uint32{0, 1}, nil, nil, nil)
	if !IsUnsupported(err) {
		t.Fatalf("pattern outside the subset: %v", err)
	}
}
