package bloomgpu

import "testing"

// MatchRowsMany: two queries over one table of distinct conditions in one call; every plane equals MatchRows for its query alone, a
// set's mask switches a query off on that set's rows, and the call's limits answer IsUnsupported.  Needs a gfx950 device; skipped
// otherwise.
func TestMatchRowsMany(t *testing.T) {
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
	// table: 0 = FieldToken(level, error), 1 = FieldToken(service, payment); query 0 = And(0, 1), query 1 = 1, query 2 = nil
	conds := []MatchCond{{Kind: KindFieldToken, Field: "level", Token: "error"}, {Kind: KindFieldToken, Field: "service", Token: "payment"}}
	progOps := []uint32{OpTerm<<28 | 0, OpTerm<<28 | 1, OpAnd<<28 | 2, OpTerm<<28 | 1}
	progOff := []uint32{0, 3, 4, 4}
	planes, host, err := g.MatchRowsMany(rows, off, conds, progOps, progOff, nil, nil, nil)
	if err != nil || len(host) != 0 || len(planes) != 3 {
		t.Fatalf("planes %v host %v err %v", planes, host, err)
	}
	if planes[0][0] != 0b001 || planes[1][0] != 0b011 || planes[2][0] != 0b111 {
		t.Fatalf("planes %v", planes)
	}
	for q := 0; q < 3; q++ {
		one, _, err := g.MatchRows(rows, off, conds, progOps[progOff[q]:progOff[q+1]])
		if err != nil || one[0] != planes[q][0] {
			t.Fatalf("query %d: single call %v err %v, plane %v", q, one, err, planes[q])
		}
	}
	// two sets: rows {0, 1} evaluate query 1 only, row {2} queries 0 and 2
	planes, host, err = g.MatchRowsMany(rows, off, conds, progOps, progOff, []uint32{0, 2, 3}, []uint64{0b010, 0b101}, nil)
	if err != nil || len(host) != 0 {
		t.Fatalf("masked: host %v err %v", host, err)
	}
	if planes[0][0] != 0 || planes[1][0] != 0b011 || planes[2][0] != 0b100 {
		t.Fatalf("masked planes %v", planes)
	}
	// a FieldRegex condition is not part of the batched call
	_, _, err = g.MatchRowsMany(rows, off, []MatchCond{{Kind: KindFieldRegex, Field: "level", Token: "err"}}, []uint32{OpTerm << 28}, []uint32{0, 1}, nil, nil, nil)
	if !IsUnsupported(err) {
		t.Fatalf("regex kind: %v", err)
	}
	// ... nor are 65 queries
	_, _, err = g.MatchRowsMany(rows, off, conds, nil, make([]uint32, 66), nil, nil, nil)
	if !IsUnsupported(err) {
		t.Fatalf("65 queries: %v", err)
	}
}
